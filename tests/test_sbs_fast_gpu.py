"""HipGenerator.sample_distinct(prefix, width, fast=True) -- the bf16 fast distinct names (Generator::distinct_fast,
docs/DESIGN.md §4i) -- against the float64 twin of models/sbs_fast_ref.py.

For every prefix: sbs_ref.check_result's invariants (rows distinct, gumbel non-increasing from exactly 0, prefix /
padding / EOS placement, dead slots) and logq within the sum over the row's free tokens of 2 D + 1e-5 +
2e-7 exp(-ref) of cpu_ref.score(rows, temperature=, prefix=, round_operands=True) in float64, D = the case's
largest |twin - exact| name_logp over the twin's rows and the returned ones.  Rows, n_tok and n_found are compared
with the twin's only for prefixes whose every step's scaled clearance is at least 2 D; there gumbel is within
(n_tok 2 D + ATOL["Gt"]) times the twin's scale."""
import numpy as np
import pytest

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import sbs_fast_ref as sf
from gru_mpi_cuda_amd.models import sbs_ref
from gru_mpi_cuda_amd.models.params import init_params

pytestmark = pytest.mark.gpu
KEYS = ("rows", "logq", "gumbel", "n_tok", "n_found")


def _gen(case, **kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = sf.case_model(case)
    return HipGenerator(cfg, p, precision="bf16", **kw)


@pytest.mark.parametrize("case", sf.CASES, ids=lambda c: c.name)
def test_distinct_fast_matches_the_twin(case):
    cfg, p = sf.case_model(case)
    t = sf.twin(case)
    gen = _gen(case, max_batch=64)
    res = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **sf.case_kwargs(case))
    assert gen.g.read_error() == 0 and not gen.g.distinct_last_persist()
    # invariants for every prefix; nothing counts as settled here (the twin's bytes are compared below)
    none = dict(t, settled=np.zeros(len(case.prefixes), bool))
    assert sbs_ref.check_result(cfg, case.prefixes, none, res) == []
    D = max(t["D"], sf.rows_D(p, cfg, case, res.rows, res.n_found))
    ref, bound = sf.logq_bound(p, cfg, case, res.rows, res.n_found, res.n_tok, D)
    live = np.arange(case.W)[None, :] < res.n_found[:, None]
    d = np.abs(res.logq.astype(np.float64) - ref)
    s = t["clear"].min(1) >= 2 * D
    free = live & (bound > 0)       # a row without a free token has logq 0 and bound 0
    print(f"{case.name}: D {D:.3e}, max |d| {d[live].max():.3e}, max d/bound {(d[free] / bound[free]).max():.3f}, "
          f"settled {int(s.sum())} of {len(case.prefixes)}")
    assert np.all(d[live] <= bound[live])
    assert 2 * int((~s).sum()) <= len(case.prefixes)
    assert np.array_equal(res.rows[s], t["rows"][s]) and np.array_equal(res.n_tok[s], t["n_tok"][s])
    assert np.array_equal(res.n_found[s], t["n_found"][s])
    lv = live[s]
    with np.errstate(invalid="ignore"):      # dead slots: -inf on both sides
        dg = np.abs(res.gumbel[s].astype(np.float64) - t["gumbel"][s])[lv]
    tol = ((t["n_tok"][s] * 2 * D + sbs_ref.ATOL["Gt"]) * t["scale"][s][:, None])[lv]
    print(f"{case.name}: gumbel max |d| {dg.max() if dg.size else 0:.3e}, largest scale {t['scale'].max():.3g}")
    assert np.all(dg <= tol)


def test_replay_eager_and_other_prefixes():
    case = next(c for c in sf.CASES if c.name == "L2-V64-W3-T0.7")
    kw = sf.case_kwargs(case)
    gen = _gen(case, max_batch=64)
    first = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **kw)
    assert gen.g.distinct_fast_graphs() == 1 and gen.g.beam_workspace_bytes() > 0
    again = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **kw)        # a replay
    moved = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **dict(kw, seed=kw["seed"] + 1))
    # the same count, the prefixes reversed: name n keeps its noise when it keeps its global index
    halves = [gen.sample_distinct([q], case.W, fast=True, **dict(kw, start=kw["start"] + n)) for n, q in
              list(enumerate(case.prefixes))[::-1][:3]]
    assert gen.g.distinct_fast_graphs() == 2      # (10, W) and (1, W): seed, start and 1 / T are not baked in
    gen.g.set_use_graph(False)
    eager = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **kw)
    for k in KEYS:
        assert getattr(first, k).tobytes() == getattr(again, k).tobytes() == getattr(eager, k).tobytes(), k
        for i, h in enumerate(halves):
            assert getattr(h, k)[0].tobytes() == getattr(first, k)[len(case.prefixes) - 1 - i].tobytes(), k
    assert moved.gumbel.tobytes() != first.gumbel.tobytes()


def test_exact_path_keeps_its_bytes():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    case = next(c for c in sf.CASES if c.name == "L2-V64-W3")
    cfg, p = sf.case_model(case)
    kw = sf.case_kwargs(case)
    exact = HipGenerator(cfg, p, precision="fp32", max_batch=64)
    before = exact.sample_distinct(list(case.prefixes), case.W, **kw)
    gen = _gen(case, max_batch=64)
    fast = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **kw)
    beam = gen.beam_search(list(case.prefixes), case.W, fast=True)       # shares the loop's buffers
    fast2 = gen.sample_distinct(list(case.prefixes), case.W, fast=True, **kw)
    after = exact.sample_distinct(list(case.prefixes), case.W, **kw)
    for k in KEYS:
        assert getattr(before, k).tobytes() == getattr(after, k).tobytes(), k
        assert getattr(fast, k).tobytes() == getattr(fast2, k).tobytes(), k
    assert beam.n_beams.min() >= 1
    assert fast.logq.tobytes() != before.logq.tobytes()      # another arithmetic
    with pytest.raises(ValueError):                          # the exact call still refuses a bf16 generator
        gen.sample_distinct(list(case.prefixes), case.W, **kw)


@pytest.mark.parametrize("precision,vocab,kw", [
    ("fp32", 64, {}), ("bf16x3", 64, {}), ("bf16", 64, dict(constraints=dict(pattern="[0-9]"))), ("bf16", 96, {}),
])
def test_distinct_fast_refusals(precision, vocab, kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=vocab, embed=64, hidden=64, layers=1, max_len=4, sos=0, eos=0, seed=6)
    with pytest.raises(ValueError):
        gen = HipGenerator(cfg, init_params(cfg), max_batch=64, precision=precision)
        gen.sample_distinct(["0"], 3, fast=True, **kw)
    if vocab % 64 == 0:
        assert gen.g.distinct_fast_graphs() == 0 and gen.g.beam_workspace_bytes() == 0

"""Constrained batches through the constrained persistent launch (docs/DESIGN.md §4e / §4g), engine level:
HipGenerator with ``persist_constraints`` on the CFG, the mixtures, the oracles and the bar of
tests/test_constraints_gpu.py and tests/test_automaton_gpu.py.  The switch is off by default (those two
files assert the per-char graph for a constrained 40-name batch); here it is on."""
import re

import numpy as np
import pytest

import test_automaton_gpu as ag
import test_constraints_gpu as cg
import test_sampling_ctl_gpu as sc
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

pytestmark = pytest.mark.gpu
CFG, BAR = sc.CFG, sc.BAR


@pytest.fixture
def gp(ext):
    if ext.device_info()["cus"] < 256:
        pytest.skip("the persistent generator needs 256 compute units")
    return ext


def paths(g):
    return g.persist_con_launches(), g.ctl_graphs(), g.automaton_graphs(), g.ctl_workspace_bytes()


def test_switch_is_off_by_default_and_follows_its_setters(gp):
    gen = sc.make_gen()
    g = gen.g
    assert not g.uses_persist_con(1, False) and not g.uses_persist_con(40, True) and g.persist_con_launches() == 0
    gen.set_persist_constraints(64)
    assert all(g.uses_persist_con(n, a) for n in (1, 40, 64) for a in (False, True)) and not g.uses_persist_con(65, False)
    gen.set_persist_constraints(8)
    assert g.uses_persist_con(8, True) and not g.uses_persist_con(9, True) and g.uses_persist_ctl(9)
    g.set_persist_ctl_max(4)                                      # never beyond the controlled launch's own limit
    assert g.uses_persist_con(4, False) and not g.uses_persist_con(5, False)
    g.set_persist_ctl_max(64)
    g.set_persist(False)
    assert not g.uses_persist_con(4, False)
    assert sc.make_gen(persist_constraints=16).g.uses_persist_con(16, True)
    with pytest.raises(ValueError):
        gen.set_persist_constraints(-1)
    with pytest.raises(ValueError):                               # bf16 mode still raises
        sc.make_gen(precision="bf16", persist_constraints=64).generate(
            random_floats(4, CFG.max_len, seed=1), constraints=dict(charset="abc"))


def test_40_constrained_names_take_one_persistent_launch_per_batch_and_obey(gp):
    """A per-position mixture and an automaton mixture with the switch at 64: one constrained launch per
    batch, no recording, no staging arena; then the switch off in the same generator: the graph again;
    unconstrained plain and controlled calls before and after: their bytes, their paths."""
    N = 40
    rf = random_floats(N, CFG.max_len, seed=9)
    gen = sc.make_gen(persist_constraints=64)
    g = gen.g
    before = gen.generate(rf)
    before_ctl = gen.generate(rf, temperature=0.7, prefix="Jo")
    assert paths(g) == (0, 0, 0, 0)
    # per-position
    cons = cpu_ref.make_constraints(CFG, N, **cg.mixture(N))
    got = gen.generate(rf, constraints=cons)
    assert g.read_error() == 0 and paths(g) == (1, 0, 0, 0)
    assert cg.all_obey(got, cons)                                 # 100 %, no tolerance
    assert (gen.generate(rf, constraints=cg.mixture(N)) == got).all() and paths(g) == (2, 0, 0, 0)
    mix = gen.generate(rf, temperature=0.8, top_k=3, prefix="M", constraints=dict(pattern="M[aeiou]", charset=cg.LETTERS, max_len=6))
    assert cg.all_obey(mix, cpu_ref.make_constraints(CFG, N, pattern="M[aeiou]", charset=cg.LETTERS, max_len=6))
    assert paths(g) == (3, 0, 0, 0)
    # automaton
    kind, acons, ctl = ag.mixture(N)
    agot = gen.generate(rf, constraints=acons, **ctl)
    assert g.read_error() == 0 and paths(g) == (4, 0, 0, 0)
    assert ag.all_in_language(agot, kind, ctl) is None            # Python's re on the whole name
    assert (gen.generate(rf, constraints=acons, **ctl) == agot).all() and paths(g) == (5, 0, 0, 0)
    print("40 names identical to the fp64 oracle: per-position", sc.same(got, sc.oracle(("cons40", 0), False, rf, constraints=cg.mixture(N))),
          "automaton", sc.same(agot, sc.oracle(("aut40", 0), False, rf, constraints=acons, **ctl)))
    # the other paths: untouched
    assert g.uses_persist(N) and (gen.generate(rf) == before).all()
    assert (gen.generate(rf, temperature=0.7, prefix="Jo") == before_ctl).all() and paths(g) == (5, 0, 0, 0)
    # the switch off in the same generator: the per-char graphs, rows that obey
    gen.set_persist_constraints(0)
    off = gen.generate(rf, constraints=cons)
    assert paths(g)[:3] == (5, 1, 0) and g.ctl_workspace_bytes() > 0 and cg.all_obey(off, cons)
    aoff = gen.generate(rf, constraints=acons, **ctl)
    assert paths(g)[:3] == (5, 1, 1) and ag.all_in_language(aoff, kind, ctl) is None
    # ... and on again
    gen.set_persist_constraints(64)
    assert (gen.generate(rf, constraints=cons) == got).all() and (gen.generate(rf, constraints=acons, **ctl) == agot).all()
    assert paths(g)[:3] == (7, 1, 1) and g.read_error() == 0
    assert (gen.generate(rf) == before).all()


def test_1000_names_in_persistent_batches_match_the_fp64_oracles(gp):
    """max_batch = 64: fifteen batches of 64 names and one of 40, each one constrained persistent launch on
    the caller's arrays at the batch's rows (a batch that read rows 0.. would follow another name's
    constraint: the mixtures depend on the batch)."""
    N = 1000
    rf = random_floats(N, CFG.max_len, seed=9)
    gen = sc.make_gen(max_batch=64, persist_constraints=64)
    g = gen.g
    kw = cg.mixture(N)
    cons = cpu_ref.make_constraints(CFG, N, **kw)
    got = gen.generate(rf, constraints=cons)
    assert g.read_error() == 0 and paths(g) == (16, 0, 0, 0) and cg.all_obey(got, cons)
    s = sc.same(got, sc.oracle(("cons1000", 0), False, rf, constraints=kw))
    print("constrained names (persistent) identical to the fp64 oracle:", s)
    assert s >= BAR
    kind, acons, ctl = ag.mixture(N)
    agot = gen.generate(rf, constraints=acons, **ctl)
    assert g.read_error() == 0 and paths(g) == (32, 0, 0, 0) and ag.all_in_language(agot, kind, ctl) is None
    s = sc.same(agot, sc.oracle(("aut1000", 0), False, rf, constraints=acons, **ctl))
    print("automaton-constrained names (persistent) identical to the fp64 oracle:", s)
    assert s >= BAR


def test_batches_larger_than_the_switch_go_to_the_graph(gp):
    N = 100
    rf = random_floats(N, CFG.max_len, seed=9)
    gen = sc.make_gen(persist_constraints=64)                     # max_batch 4096: one batch of 100 names
    cons = cpu_ref.make_constraints(CFG, N, **cg.mixture(N))
    got = gen.generate(rf, constraints=cons)
    assert paths(gen.g)[:3] == (0, 1, 0) and cg.all_obey(got, cons)
    kind, acons, ctl = ag.mixture(N)
    agot = gen.generate(rf, constraints=acons, **ctl)
    assert paths(gen.g)[:3] == (0, 1, 1) and ag.all_in_language(agot, kind, ctl) is None
    # a switch below the batch: the graph as well
    gen.set_persist_constraints(16)
    rf40 = rf[:40 * CFG.max_len]
    gen.generate(rf40, constraints=dict(charset="abc"))
    assert paths(gen.g)[:3] == (0, 2, 1)
    gen.generate(rf[:16 * CFG.max_len], constraints=dict(charset="abc"))
    assert paths(gen.g)[:3] == (1, 2, 1) and gen.g.read_error() == 0


def test_an_unsupported_shape_takes_the_graph_and_obeys(gp):
    """H = 64: no persistent variant at all."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=256, embed=64, hidden=64, layers=1, max_len=10, sos=0, eos=0, seed=5)
    gen = HipGenerator(cfg, init_params(cfg), precision="fp32", persist_constraints=64)
    N = 20
    assert not gen.g.uses_persist_con(N, False) and not gen.g.uses_persist_con(N, True)
    rf = random_floats(N, cfg.max_len, seed=3)
    got = gen.generate(rf, constraints=dict(regex="[A-Z][a-z]{3,6}"))
    assert paths(gen.g)[:3] == (0, 0, 1) and gen.g.read_error() == 0
    assert all(re.fullmatch("[A-Z][a-z]{3,6}", bytes(r[:cfg.max_len]).split(b"\0")[0].decode("latin-1")) for r in got)
    cons = cpu_ref.make_constraints(cfg, N, pattern="[A-Z]", charset=cg.LOWER, min_len=4, max_len=7)
    assert cg.all_obey(gen.generate(rf, constraints=cons), cons) and paths(gen.g)[:3] == (0, 1, 1)


def test_spin_limit_falls_back_to_the_constrained_graph(gp):
    """The hook of test_generator_spin_limit_falls_back_to_the_controlled_graph: the constrained launch
    starts with its spin-limit bit set, the batch is regenerated on the per-char graph and obeys."""
    N = 40
    rf = random_floats(N, CFG.max_len, seed=13)
    kind, acons, ctl = ag.mixture(N)
    ref = sc.make_gen()
    ref.g.set_persist(False)
    want = ref.generate(rf, constraints=acons, **ctl)
    gen = sc.make_gen(persist_constraints=64)
    assert gen.g.uses_persist_con(N, True)
    gen.g.inject_persist_error()
    got = gen.generate(rf, constraints=acons, **ctl)
    assert (got == want).all() and ag.all_in_language(got, kind, ctl) is None
    assert gen.g.read_error() == 0 and not gen.g.uses_persist_con(N, True) and not gen.g.uses_persist(N)
    assert paths(gen.g)[:3] == (1, 0, 1) and gen.g.ctl_workspace_bytes() > 0
    cons = cpu_ref.make_constraints(CFG, N, **cg.mixture(N))      # the path is off now: the graph
    assert cg.all_obey(gen.generate(rf, constraints=cons), cons) and paths(gen.g)[:3] == (1, 1, 1)


def test_cli_generate_persist_constraints(gp, tmp_path):
    from gru_mpi_cuda_amd import cli
    from gru_mpi_cuda_amd.utils import ckpt
    m = str(tmp_path / "model.bin")
    ckpt.save(m, CFG, sc.model())
    for flags in (["--persist-constraints"], ["--persist-constraints", "32"]):
        out = str(tmp_path / "names.txt")
        assert cli.main(["generate", "--ckpt", m, "-n", "20", "--seed", "3", "--regex", ".*son", "--charset", cg.LETTERS,
                         *flags, "--temperature", "0.8", "--top-k", "40", "--top-p", "0.95", "--out", out]) == 0
        names = open(out).read().splitlines()
        assert len(names) == 20 and all(re.fullmatch("[A-Za-z]*son", nm) for nm in names), names
    # the keyword reaches the generator through namegen; the CPU path ignores it
    from gru_mpi_cuda_amd.engine import generator as G
    G.namegen_initialize(20, 3, m, None, "gen")
    try:
        buf = np.zeros(20 * (CFG.max_len + 1), np.uint8)
        G.namegen(20, random_floats(20, CFG.max_len, seed=3), buf, constraints=dict(regex=".*son", charset=cg.LETTERS),
                  persist_constraints=64)
        assert G._S.gen.g.persist_con_launches() == 1 and G._S.gen.g.automaton_graphs() == 0
        assert all(re.fullmatch("[A-Za-z]*son", nm) for nm in G.decode_names(buf, 20, CFG.max_len))
    finally:
        G.namegen_finalize()
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "4", "--regex", ".*son", "--persist-constraints",
                     "--out", str(tmp_path / "cpu.txt")]) == 0

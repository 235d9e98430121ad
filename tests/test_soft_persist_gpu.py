"""Soft batches through the soft persistent launch (docs/DESIGN.md §4h), engine level: HipGenerator with
``persist_soft`` on the CFG, the oracles and the bar of tests/test_sampling_ctl_gpu.py, with the settings of
tests/test_gen_soft_ref.py (which shows fp32 cpu_ref alone to stay at the bar on them).  The switch is off by
default (tests/test_soft_ctl_gpu.py asserts the per-char graph for every soft batch); here it is on."""
import re

import numpy as np
import pytest

import test_constraints_gpu as cg
import test_gen_soft_ref as tsr
import test_sampling_ctl_gpu as sc
import test_soft_ctl as ts
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

pytestmark = pytest.mark.gpu
CFG, BAR = sc.CFG, sc.BAR
NONE, MASK, AUTO = 0, 1, 2
REGEX = "[A-Z][a-z]+(son|sen)?"


@pytest.fixture
def gp(ext):
    if ext.device_info()["cus"] < 256:
        pytest.skip("the persistent generator needs 256 compute units")
    return ext


def paths(g):
    return g.persist_soft_launches(), g.soft_graphs(), g.ctl_graphs(), g.automaton_graphs(), g.ctl_workspace_bytes()


def names_of(rows):
    return [bytes(r[:CFG.max_len]).split(b"\0")[0].decode("latin-1") for r in rows]


def test_switch_is_off_by_default_and_follows_its_setters(gp):
    gen = sc.make_gen()
    g = gen.g
    assert not g.uses_persist_soft(1, NONE) and not g.uses_persist_soft(40, AUTO) and g.persist_soft_launches() == 0
    gen.set_persist_soft(64)
    assert all(g.uses_persist_soft(n, NONE) for n in (1, 40, 64)) and not g.uses_persist_soft(65, NONE)
    assert not g.uses_persist_soft(8, 3) and not g.uses_persist_soft(8, -1)
    # with constraints never beyond the constrained launch's own switch
    assert not g.uses_persist_soft(8, MASK) and not g.uses_persist_soft(8, AUTO)
    gen.set_persist_constraints(64)
    assert all(g.uses_persist_soft(n, m) for n in (1, 40, 64) for m in (MASK, AUTO))
    gen.set_persist_constraints(8)
    assert g.uses_persist_soft(8, AUTO) and not g.uses_persist_soft(9, AUTO) and g.uses_persist_soft(9, NONE)
    gen.set_persist_soft(8)
    assert g.uses_persist_soft(8, NONE) and not g.uses_persist_soft(9, NONE) and g.uses_persist_ctl(9)
    gen.set_persist_soft(64)
    g.set_persist_ctl_max(4)                                      # never beyond the controlled launch's own limit
    assert g.uses_persist_soft(4, NONE) and not g.uses_persist_soft(5, NONE)
    g.set_persist_ctl_max(64)
    g.set_persist(False)
    assert not g.uses_persist_soft(4, NONE)
    assert sc.make_gen(persist_soft=16).g.uses_persist_soft(16, NONE)
    with pytest.raises(ValueError):
        gen.set_persist_soft(-1)
    with pytest.raises(ValueError):                               # bf16 mode still raises
        sc.make_gen(precision="bf16", persist_soft=64).generate(random_floats(4, CFG.max_len, seed=1), presence_penalty=0.5)


def test_40_soft_names_take_one_persistent_launch_per_batch(gp):
    """Soft alone, with per-position constraints and with a regex, the switch at 64: one soft launch per batch,
    no recording, no staging arena; then the switch off in the same generator: the graph again; on again: the
    bytes of before; plain and controlled calls before and after: their bytes, their paths."""
    N = 40
    gen = sc.make_gen(persist_soft=64, persist_constraints=64)
    g = gen.g
    rf9 = random_floats(N, CFG.max_len, seed=9)
    before = gen.generate(rf9)
    before_ctl = gen.generate(rf9, temperature=0.7, prefix="Jo")
    assert paths(g) == (0, 0, 0, 0, 0) and g.persist_con_launches() == 0
    got = {}
    for i, case in enumerate(("sampled", "pattern", "regex")):
        kw = ts.soft_cases(N)[case]
        rf = random_floats(N, CFG.max_len, seed=ts.SEEDS[case])
        got[case] = gen.generate(rf, **kw)
        assert g.read_error() == 0 and paths(g) == (2 * i + 1, 0, 0, 0, 0), case
        want = cpu_ref.generate(ts.f64(sc.model()), CFG, rf, **kw)
        print(f"40 soft names ({case}) identical to the fp64 oracle: {sc.same(got[case], want)}")
        assert sc.same(got[case], want) >= 0.9                    # (40 names: one name is 2.5 %; the bar is taken at 200 below)
        assert (gen.generate(rf, **kw) == got[case]).all() and paths(g) == (2 * i + 2, 0, 0, 0, 0)
    launches = g.persist_soft_launches()
    assert launches == 6 and g.persist_con_launches() == 0        # soft launches are counted as such
    assert all(re.fullmatch(REGEX, nm) for nm in names_of(got["regex"]))
    assert cg.all_obey(got["pattern"], cpu_ref.make_constraints(CFG, N, **ts.soft_cases(N)["pattern"]["constraints"]))
    # the other paths: untouched
    assert (gen.generate(rf9) == before).all() and (gen.generate(rf9, temperature=0.7, prefix="Jo") == before_ctl).all()
    assert paths(g) == (launches, 0, 0, 0, 0)
    # the switch off in the same generator: the per-char soft graphs
    gen.set_persist_soft(0)
    off = {}
    for case in ("sampled", "pattern", "regex"):
        off[case] = gen.generate(random_floats(N, CFG.max_len, seed=ts.SEEDS[case]), **ts.soft_cases(N)[case])
    assert paths(g)[:4] == (launches, 3, 0, 0) and g.ctl_workspace_bytes() > 0 and g.read_error() == 0
    assert all(sc.same(off[case], got[case]) >= 0.9 for case in off)
    # ... and on again
    gen.set_persist_soft(64)
    for case in ("sampled", "pattern", "regex"):
        again = gen.generate(random_floats(N, CFG.max_len, seed=ts.SEEDS[case]), **ts.soft_cases(N)[case])
        assert (again == got[case]).all(), case
    assert paths(g)[:4] == (launches + 3, 3, 0, 0) and g.read_error() == 0
    assert (gen.generate(rf9) == before).all() and (gen.generate(rf9, temperature=0.7, prefix="Jo") == before_ctl).all()


@pytest.mark.parametrize("case", sorted(tsr.ENGINE_SEEDS))
def test_200_names_in_persistent_batches_match_the_fp64_oracle(gp, case):
    """max_batch = 64: three batches of 64 names and one of 8, each one soft persistent launch on the caller's
    arrays at the batch's rows (the names' bias lines and penalties depend on the row and on the batch: a batch
    that read rows 0.. would show)."""
    N = tsr.ENGINE_N
    rf, want = tsr.engine_oracle(case)
    kw = tsr.engine_cases(N)[case]
    gen = sc.make_gen(max_batch=64, persist_soft=64, persist_constraints=64)
    got = gen.generate(rf, **kw)
    assert gen.g.read_error() == 0 and paths(gen.g) == (4, 0, 0, 0, 0)
    if case == "pattern":      # inside the constraint at 100 %, no tolerance
        assert cg.all_obey(got, cpu_ref.make_constraints(CFG, N, **kw["constraints"]))
    if case == "regex":
        assert all(re.fullmatch(REGEX, nm) and len(nm) <= 8 for nm in names_of(got))
    s = sc.same(got, want)
    print(f"soft names (persistent, {case}) identical to the fp64 oracle: {s}")
    assert s >= BAR
    hard = {k: v for k, v in kw.items() if k not in ("logit_bias", "presence_penalty", "frequency_penalty")}
    assert not (gen.generate(rf, **hard) == got).all()            # the soft values matter


def test_a_huge_presence_penalty_leaves_no_repeated_char(gp):
    N = 40
    gen = sc.make_gen(persist_soft=64)
    rows = gen.generate(random_floats(N, CFG.max_len, seed=5), presence_penalty=1e4, logit_bias={0: -2.0})
    assert gen.g.persist_soft_launches() == 1 and gen.g.read_error() == 0
    names = names_of(rows)
    assert all(len(set(nm)) == len(nm) for nm in names) and max(len(nm) for nm in names) >= 5, names


def test_batches_larger_than_the_switch_and_other_vocabularies_go_to_the_graph(gp):
    N = 100
    rf = random_floats(N, CFG.max_len, seed=9)
    kw = dict(logit_bias={"e": 1.0}, frequency_penalty=0.5)
    gen = sc.make_gen(persist_soft=64)                            # max_batch 4096: one batch of 100 names
    gen.generate(rf, **kw)
    assert paths(gen.g)[:2] == (0, 1)
    gen.set_persist_soft(16)                                      # a switch below the batch: the graph as well
    gen.generate(rf[:40 * CFG.max_len], **kw)
    assert paths(gen.g)[:2] == (0, 2)
    a = gen.generate(rf[:16 * CFG.max_len], **kw)
    assert paths(gen.g)[:2] == (1, 2) and gen.g.read_error() == 0
    gen.set_persist_soft(0)
    assert sc.same(gen.generate(rf[:16 * CFG.max_len], **kw), a) >= 0.9
    # a constrained soft batch needs the constrained switch as well
    gen.set_persist_soft(64)
    gen.generate(rf[:16 * CFG.max_len], constraints=dict(charset="abc"), **kw)
    assert gen.g.persist_soft_launches() == 1
    gen.set_persist_constraints(64)
    gen.generate(rf[:16 * CFG.max_len], constraints=dict(charset="abc"), **kw)
    assert gen.g.persist_soft_launches() == 2 and gen.g.persist_con_launches() == 0
    # V = 512 (a bias alone: the penalties need vocab <= 256) stays on the graph: documented, not an error
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=512, embed=64, hidden=256, layers=1, max_len=8, sos=0, eos=0, seed=6)
    wide = HipGenerator(cfg, init_params(cfg), precision="fp32", persist_soft=64)
    assert wide.g.uses_persist_ctl(8) and not wide.g.uses_persist_soft(8, NONE)
    rows = wide.generate(random_floats(8, cfg.max_len, seed=3), logit_bias={"a": 1.0})
    want = cpu_ref.generate({k: v.double() for k, v in init_params(cfg).items()}, cfg, random_floats(8, cfg.max_len, seed=3),
                            logit_bias={"a": 1.0})
    assert paths(wide.g)[:2] == (0, 1) and wide.g.read_error() == 0 and sc.same(rows, want) >= 0.75


def test_an_unsupported_shape_takes_the_graph(gp):
    """H = 64: no persistent variant at all."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=256, embed=64, hidden=64, layers=1, max_len=10, sos=0, eos=0, seed=5)
    gen = HipGenerator(cfg, init_params(cfg), precision="fp32", persist_soft=64, persist_constraints=64)
    N = 20
    assert not any(gen.g.uses_persist_soft(N, m) for m in (NONE, MASK, AUTO))
    rf = random_floats(N, cfg.max_len, seed=3)
    kw = dict(presence_penalty=1.0, logit_bias={"xqz": -2.0})
    got = gen.generate(rf, **kw)
    want = cpu_ref.generate({k: v.double() for k, v in init_params(cfg).items()}, cfg, rf, **kw)
    assert paths(gen.g)[:2] == (0, 1) and gen.g.read_error() == 0 and sc.same(got, want) >= 0.9


@pytest.mark.parametrize("case", ["sampled", "regex"])
def test_spin_limit_falls_back_to_the_soft_graph(gp, case):
    """The hook of test_generator_spin_limit_falls_back_to_the_controlled_graph: the soft launch starts with
    its spin-limit bit set, the batch is regenerated on the per-char soft graph -- the bias table and, with a
    regex, the automaton tables staged late -- and its rows are that graph's."""
    N = 40
    kw = ts.soft_cases(N)[case]
    rf = random_floats(N, CFG.max_len, seed=ts.SEEDS[case])
    ref = sc.make_gen()
    ref.g.set_persist(False)
    want = ref.generate(rf, **kw)
    gen = sc.make_gen(persist_soft=64, persist_constraints=64)
    mode = AUTO if case == "regex" else NONE
    assert gen.g.uses_persist_soft(N, mode)
    gen.g.inject_persist_error()
    got = gen.generate(rf, **kw)
    assert (got == want).all()
    assert gen.g.read_error() == 0 and not gen.g.uses_persist_soft(N, mode) and not gen.g.uses_persist(N)
    assert paths(gen.g)[:4] == (1, 1, 0, 0) and gen.g.ctl_workspace_bytes() > 0
    if case == "regex":
        assert all(re.fullmatch(REGEX, nm) for nm in names_of(got))
    assert (gen.generate(rf, **kw) == want).all() and paths(gen.g)[:2] == (1, 1)      # the path is off now: the graph


def test_cli_generate_persist_soft(gp, tmp_path):
    from gru_mpi_cuda_amd import cli
    from gru_mpi_cuda_amd.utils import ckpt
    m = str(tmp_path / "model.bin")
    ckpt.save(m, CFG, sc.model())
    outs = []
    for flags in ([], ["--persist-soft"], ["--persist-soft", "32"]):
        out = str(tmp_path / f"names{len(outs)}.txt")
        assert cli.main(["generate", "--ckpt", m, "-n", "20", "--seed", "3", "--logit-bias", "xqz=-2", "--eos-bias", "-1",
                         "--presence-penalty", "0.5", "--frequency-penalty", "0.5", *flags, "--temperature", "0.8",
                         "--top-k", "40", "--top-p", "0.95", "--out", out]) == 0
        outs.append(open(out).read().splitlines())
        assert len(outs[-1]) == 20
    assert outs[1] == outs[2] and sum(a == b for a, b in zip(outs[0], outs[1])) >= 18
    with pytest.raises(SystemExit):
        cli.main(["generate", "--ckpt", m, "-n", "4", "--presence-penalty", "0.5", "--persist-soft", "-1"])
    # the keyword reaches the generator through namegen; the CPU path ignores it
    from gru_mpi_cuda_amd.engine import generator as G
    G.namegen_initialize(20, 3, m, None, "gen")
    try:
        buf = np.zeros(20 * (CFG.max_len + 1), np.uint8)
        G.namegen(20, random_floats(20, CFG.max_len, seed=3), buf, presence_penalty=0.5, persist_soft=64)
        assert G._S.gen.g.persist_soft_launches() == 1 and G._S.gen.g.soft_graphs() == 0
        G.namegen(20, random_floats(20, CFG.max_len, seed=3), buf, presence_penalty=0.5, persist_soft=0)
        assert G._S.gen.g.persist_soft_launches() == 1 and G._S.gen.g.soft_graphs() == 1
    finally:
        G.namegen_finalize()
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "4", "--presence-penalty", "0.5", "--persist-soft",
                     "--out", str(tmp_path / "cpu.txt")]) == 0

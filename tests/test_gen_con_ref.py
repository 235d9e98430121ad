"""CPU tests of models/gen_con_ref.py, the reference of the persistent generator's constrained launch:
with a free table it is gen_ctl_ref's trajectory, its rows stay inside their sets, the planter stays
within its cap of moved names, the float32 emulator alone passes every check that
tests/test_gen_persist_con_gpu.py makes of a launch, and every planted defect (gen_con_ref.MUTATIONS)
fails that same checker on the case named for it."""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import gen_con_ref as nr
from gru_mpi_cuda_amd.models import gen_ctl_ref as cr
from gru_mpi_cuda_amd.models import gen_ref as gr

CASE = {c.name: c for c in nr.CON_CASES}


@functools.lru_cache(maxsize=None)
def setup(name):
    return nr.case_setup(CASE[name])


def test_case_list_is_the_issue_s():
    for m in ("mask", "auto"):
        n = [c for c in nr.CASES_N if c.mode == m]
        assert [c.ctl.N for c in n] == [1, 8, 9, 16, 17, 33] and all((c.ctl.H, c.ctl.L, c.ctl.ML) == (256, 1, 4) for c in n)
        assert [(c.ctl.H, c.ctl.L, c.ctl.N) for c in nr.CASES_T if c.mode == m] == [(1024, 2, 1), (1024, 2, 17)]
        assert all((c.ctl.H, c.ctl.L, c.ctl.V) == (256, 2, 512) for c in nr.CASES_V)
        assert {(c.ctl.H, c.ctl.L) for c in nr.CASES_A if c.mode == m} == set(gr.VARIANTS)
        assert {(c.ctl.H, c.ctl.L) for c in nr.CASES_A512 if c.mode == m} == set(cr.V512)
        assert all(c.ctl.N == 3 for c in nr.CASES_A + nr.CASES_A512)
    assert len(CASE) == len(nr.CON_CASES)


def test_pack_is_the_table_layout():
    bits = np.zeros((2, 256), dtype=bool)
    bits[0, [0, 31, 32, 255]] = True
    bits[1, 70] = True
    tab = nr.pack(bits)
    assert tab.shape == (2, 8) and tab.dtype == np.uint32
    assert tab[0, 0] == (1 | 1 << 31) and tab[0, 1] == 1 and tab[0, 7] == 1 << 31 and tab[1, 2] == 1 << 6
    assert np.array_equal(nr.unpack(tab, 256), bits)


@pytest.mark.parametrize("name", ["mask-n-N17", "auto-n-N17", "mask-v512-N20", "auto-g-N20-ends-probs"])
def test_tables_hold_what_can_go_wrong(name):
    c = CASE[name]
    d, ctl, con, orc = setup(name)
    V, ML, N = c.ctl.V, c.ctl.ML, c.ctl.N
    assert not con["bits"][:, V - nr.TAIL:].any() and con["bits"].any(-1).all()
    assert not orc["oob"].any()
    assert (orc["line"] == con["rows"] - 1).any(), "the last line / state is not in use"
    if c.mode == "auto":
        assert con["rows"] == nr.AUTO_STATES and (con["nxt"][:, c.ctl.eos] == 0).all() and con["nxt"].max() == con["rows"] - 1
    free = orc["sampled_step"]
    if c.kind == "rich":
        # a set of exactly one char: the pick is that char under every control mixture of the launch
        one = np.isin(orc["line"], con["single"])
        assert one[1].all() and (con["bits"][con["single"]].sum(-1) == 1).all()
        for t, n in np.argwhere(one & ~(np.arange(ML)[:, None] < ctl["plen"][None, :])):
            assert con["bits"][orc["line"][t, n], orc["sampled"][t, n]], (t, n)
        mixes = {(float(ctl["inv_temp"][n]), int(ctl["top_k"][n]), float(ctl["top_p"][n])) for n in np.flatnonzero(ctl["plen"] <= 1)}
        assert len(mixes) >= min(N, 12) - 3
        # top_k larger than the set, a prefix byte outside its set, and the fallback inside the set
        size = orc["allowed"].sum(-1)
        assert (free & (size < ctl["top_k"][None, :]) & (ctl["top_k"][None, :] < V)).any()
        forced = np.arange(ML)[:, None] < ctl["plen"][None, :]
        assert any(not orc["allowed"][t, n, ctl["prefix"][n, t]] for t, n in np.argwhere(forced))
        assert ctl["beyond"]
        for n, t in ctl["beyond"]:
            assert orc["sampled"][t, n] == np.flatnonzero(orc["keep"][t, n].numpy())[-1] < V - nr.TAIL
    if c.kind == "ends":
        assert not orc["alive_after"][1].any() and (ctl["plen"] == ML).any()      # ends inside a prefix / mid-way
        if c.mode == "auto":
            ended = np.argwhere(orc["sampled"] == c.ctl.eos)
            assert len(ended) and all(orc["state_after"][t, n] == 0 for t, n in ended)
    # every non-forced pick of every name, dead ones included, is inside its set
    forced = np.arange(ML)[:, None] < ctl["plen"][None, :]
    for t, n in np.argwhere(~forced):
        assert orc["allowed"][t, n, orc["sampled"][t, n]]
    if c.mode == "auto":
        assert np.array_equal(nr.walk(con, orc["sampled"], ML), orc["state_after"][ML - 1].astype(np.int32))


@pytest.mark.parametrize("c", nr.CASES_F, ids=lambda c: c.name)
def test_a_free_table_gives_gen_ctl_ref_s_trajectory(c):
    d, ctl, con, orc = setup(c.name)
    plain_ctl, plain = cr.plant(d, cr.controls(c.ctl))
    assert np.array_equal(plain["rf"], orc["rf"]) and plain_ctl["moved"] == ctl["moved"]
    for f64, a, b in ((True, plain, orc), (False, cr.emulate(d, plain_ctl, plain["rf"]), nr.emulate(d, ctl, con, orc["rf"]))):
        for k, v in a.items():
            x, y = (z.numpy() if torch.is_tensor(z) else np.asarray(z) for z in (v, b[k]))
            assert np.array_equal(x, y), (k, f64)


@pytest.mark.parametrize("c", nr.CON_CASES, ids=lambda c: c.name)
def test_emulator_passes_the_launch_checker(c):
    d, ctl, con, orc = setup(c.name)                              # plant asserts the guards and the cap on moved names
    assert not cr.clearance(ctl, orc) and len(ctl["moved"]) <= max(c.ctl.N // 8, 1)
    emu = nr.emulate(d, ctl, con, orc["rf"])
    assert np.array_equal(emu["out"], orc["out"]) and np.array_equal(emu["sampled"], orc["sampled"])
    assert np.array_equal(emu["state_after"], orc["state_after"])
    got = gr.synth_got(d, emu, par=len(c.name) % 2, probs=c.ctl.probs)
    fails, fig = gr.check_launch(d, orc, got, probs=c.ctl.probs, atol=nr.ATOL)
    assert not fails, fails
    if c.ctl.probs:                                               # exactly 0 outside the set at the last char (a forced one reads no mask)
        free = ctl["plen"] < c.ctl.ML
        assert (emu["probs_last"].numpy()[free][~orc["allowed"][c.ctl.ML - 1][free]] == 0).all()


def _mut_case(mut):
    name = nr.MUTATIONS[mut]
    d, ctl, con, orc = setup(name.split("+")[0])
    if name.endswith("+oob"):
        con, n, value = nr.with_oob(CASE[name.split("+")[0]], con, ctl)
        orc = nr.oracle(d, ctl, con, orc["rf"])
        assert orc["oob"][0, n] and orc["oob"].sum() == 1 and orc["line"][0, n] == 0
    return CASE[name.split("+")[0]], d, ctl, con, orc


@pytest.mark.parametrize("mut", sorted(nr.MUTATIONS))
def test_every_mutation_fails_the_launch_checker(mut):
    c, d, ctl, con, orc = _mut_case(mut)
    good = nr.emulate(d, ctl, con, orc["rf"])
    fails, _ = gr.check_launch(d, orc, gr.synth_got(d, good, probs=c.ctl.probs), probs=c.ctl.probs, atol=nr.ATOL)
    assert not fails, fails
    bad = nr.emulate(d, ctl, con, orc["rf"], mut)
    fails, fig = gr.check_launch(d, orc, gr.synth_got(d, bad, probs=c.ctl.probs), probs=c.ctl.probs, atol=nr.ATOL)
    print(f"GENCONREF {mut}: {fails[:2]}")
    assert fails, f"{mut} passes the checks of case {c.name}"


def test_mutation_list():
    assert len(nr.MUTATIONS) == 9 and {v.split("+")[0] for v in nr.MUTATIONS.values()} <= set(CASE)

"""CPU tests of models/gen_ctl_ref.py, the reference of the persistent generator's controlled launch:
with neutral controls it is gen_ref's oracle, with controls its rows are cpu_ref.generate's, the
recorded emulator deviations (which size the guards) reproduce, the float32 emulator alone passes
every check that tests/test_gen_persist_ctl_gpu.py makes of a launch, and every planted defect
(gen_ctl_ref.MUTATIONS) fails that same checker on the case named for it."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import gen_ctl_ref as cr
from gru_mpi_cuda_amd.models import gen_ref as gr
from gru_mpi_cuda_amd.models.params import init_params

CASE = {c.name: c for c in cr.CTL_CASES}


@pytest.fixture(scope="module")
def measured():
    """Every case at seeds 0, 1, 2 through the planter and the emulator.  plant asserts the guards of
    what it returns and the one-in-eight limit on moved names; measure_deviations that the emulator's
    ids, rows and kept sets are the oracle's."""
    return cr.measure_deviations(seeds=(0, 1, 2))


def test_recorded_deviations_cover_the_measured_ones(measured):
    for k, v in cr.MEASURED_DEV.items():
        print(f"GENCTLREF {k:6s} measured {measured[k]:.3e} recorded {v:.3e}")
        assert 0 < measured[k] <= v, k
        assert v <= 1.5 * measured[k] + 1e-12, f"{k}: the recorded figure is not the measured one"


def test_guards_follow_the_measured_deviations(measured):
    assert cr.GUARD_Y == 8.0 * cr.MEASURED_DEV["y"] and cr.GUARD_Y >= 8.0 * measured["y"]
    assert cr.GUARD_MASS == max(1e-4, 8.0 * cr.MEASURED_DEV["mass"]) and cr.GUARD_MASS >= 8.0 * measured["mass"]
    assert cr.ATOL["probs"] == 4.0 * cr.MEASURED_DEV["probs"]
    assert {k: v for k, v in cr.ATOL.items() if k != "probs"} == {k: v for k, v in gr.ATOL.items() if k != "probs"}


def test_case_list_is_the_issue_s():
    assert {(c.H, c.L) for c in cr.CASES_A} == set(gr.VARIANTS) and all((c.V, c.N, c.ML) == (256, 3, 4) for c in cr.CASES_A)
    assert [c.N for c in cr.CASES_B] == [1, 8, 9, 16, 17, 33] and all((c.H, c.L) == (512, 2) for c in cr.CASES_B)
    assert [c.N for c in cr.CASES_C] == [1, 8, 9, 17] and all((c.H, c.L) == (1024, 2) for c in cr.CASES_C)
    assert {(c.H, c.L) for c in cr.CASES_E} == set(cr.V512) and {c.N for c in cr.CASES_E} == {5, 33}
    assert [c.N for c in cr.CASES_N] == [1, 12, 33]
    assert len(CASE) == len(cr.CTL_CASES)
    # inside one launch of a dozen names or more: plen 0, 1 and ML, greedy, and every named cut and temperature
    for c in (CASE["cb-N16"], CASE["cb-N17"], CASE["cb-N33"], CASE["cc-N17"]):
        ctl = cr.controls(c)
        assert {0, 1, c.ML} <= set(ctl["plen"].tolist()) and (ctl["inv_temp"] == 0).any()
        assert {1, 2, 65, c.V - 1, c.V + 7} <= set(ctl["top_k"].tolist())
        assert {np.float32(1e-6), np.float32(0.5), np.float32(0.9), np.float32(1)} <= set(ctl["top_p"].tolist())
        assert {np.float32(2.0), np.float32(1.0), np.float32(0.5)} <= set(ctl["inv_temp"].tolist())
        assert ctl["beyond"]
    # every wave-uniform branch of the sampler is taken and skipped among the names of one wave's launch
    ctl = cr.controls(CASE["cb-N33"])
    free = ctl["plen"] == 0
    for taken in (ctl["plen"] > 0, ctl["inv_temp"] == 0, free & (ctl["top_k"] > 0) & (ctl["top_k"] < 256), free & (ctl["top_p"] < 1)):
        assert taken.any() and not taken.all()


@pytest.mark.parametrize("c", cr.CASES_N, ids=lambda c: c.name)
def test_neutral_controls_give_gen_ref_s_oracle(c):
    d = cr.case_inputs(c)
    ctl, run = cr.plant(d, cr.controls(c))
    assert not ctl["moved"]
    for f64, plain, mine in ((True, gr.oracle(d, run["rf"]), cr.oracle(d, ctl, run["rf"])),
                             (False, gr.emulate(d, run["rf"]), cr.emulate(d, ctl, run["rf"]))):
        for k, v in plain.items():
            a, b = (x.numpy() if torch.is_tensor(x) else np.asarray(x) for x in (v, mine[k]))
            if k in ("probs", "probs_last", "cdf") and f64:
                assert np.abs(a - b).max() <= 1e-15, k          # (torch.softmax against exp / sum)
            else:
                assert np.array_equal(a, b), (k, f64)
    assert np.array_equal(gr.plant_uniforms(d)["rf"], run["rf"])


@pytest.mark.parametrize("name", ["cb-N17", "cc-N9", "ce-H512-L1-N33", "cg-N20-full-prefix"])
def test_rows_equal_cpu_ref_generate_on_fp64_parameters(name):
    """The same model as cpu_ref parameters (an identity embedding behind W_ih0 = P^T, b_ih0 = 0), the
    same uniforms and controls: cpu_ref.generate's rows are the reference's."""
    c = CASE[name]
    d = cr.case_inputs(c)
    ctl, run = cr.plant(d, cr.controls(c))
    w = d["w64"]
    cfg = GRUConfig(vocab=c.V, embed=c.V, hidden=c.H, layers=c.L, max_len=c.ML, sos=c.sos, eos=c.eos)
    params = {"embedding": torch.eye(c.V, dtype=torch.float64), "weight_ih_l0": w["P"].T.contiguous(),
              "bias_ih_l0": torch.zeros(3 * c.H, dtype=torch.float64), "fc.weight": w["Wfc"], "fc.bias": w["bfc"]}
    for l in range(c.L):
        params[f"weight_hh_l{l}"], params[f"bias_hh_l{l}"] = w["Whh"][l], w["bhh"][l]
        if l:
            params[f"weight_ih_l{l}"], params[f"bias_ih_l{l}"] = w["Wih"][l], w["bih"][l]
    inv = ctl["inv_temp"].astype(np.float64)
    T = np.where(inv == 0, 0.0, 1.0 / np.where(inv == 0, 1.0, inv))          # 0.5, 1, 2: exact both ways
    pre = np.full((c.N, c.ML + 1), c.eos, np.uint8)               # encode_names rows: the chars, then the EOS byte
    for n in range(c.N):
        pre[n, :ctl["plen"][n]] = ctl["prefix"][n, :ctl["plen"][n]]
    made = cpu_ref.make_controls(cfg, c.N, T, ctl["top_k"], ctl["top_p"], pre)
    assert np.array_equal(made.inv_temp, ctl["inv_temp"]) and np.array_equal(made.plen, ctl["plen"])
    assert np.array_equal(made.prefix, ctl["prefix"]) and np.array_equal(made.top_p, ctl["top_p"])
    rows = cpu_ref.generate(params, cfg, run["rf"].reshape(-1), temperature=T, top_k=ctl["top_k"], top_p=ctl["top_p"], prefix=pre)
    assert np.array_equal(rows, run["out"])


@pytest.mark.parametrize("c", cr.CTL_CASES, ids=lambda c: c.name)
def test_emulator_passes_the_launch_checker(c):
    d = cr.case_inputs(c)
    ctl, orc = cr.plant(d, cr.controls(c), cr.case_plan(c))
    assert not cr.clearance(ctl, orc)
    assert np.abs(cr.oracle(d, ctl, orc["rf"])["states"].numpy() - orc["states"].numpy()).max() == 0
    emu = cr.emulate(d, ctl, orc["rf"])
    assert np.array_equal(emu["out"], orc["out"]) and np.array_equal(emu["sampled"], orc["sampled"])
    got = gr.synth_got(d, emu, par=len(c.name) % 2, probs=c.probs)
    fails, fig = gr.check_launch(d, orc, got, probs=c.probs, atol=cr.ATOL)
    assert not fails, fails
    plen, pre = ctl["plen"], ctl["prefix"]
    for n in range(c.N):                                          # the prefix is followed while the name lives
        for t in range(plen[n]):
            assert orc["sampled"][t, n] == pre[n, t]
    if c.mix == "ends":
        assert not orc["alive_after"][1].any() and (plen == c.ML).any()
        assert gr.chars_run(orc["alive_after"], c.ML, c.probs) == (c.ML if c.probs else 2)
    if c.tie:
        g = np.flatnonzero((ctl["inv_temp"] == 0) & (plen == 0))
        assert (orc["sampled"][:, g] == 5).all()                  # the lowest index of the tied maximum
        k1 = np.flatnonzero(ctl["top_k"] == 1)
        assert (orc["probs_last"][k1][:, [5, 9]].numpy() == 0.5).all()   # ties with the k-th value are all kept


@pytest.mark.parametrize("mut", sorted(cr.MUTATIONS))
def test_every_mutation_fails_the_launch_checker(mut):
    c = CASE[cr.MUTATIONS[mut]]
    d = cr.case_inputs(c)
    ctl, orc = cr.plant(d, cr.controls(c), cr.case_plan(c))
    bad = cr.emulate(d, ctl, orc["rf"], mut)
    fails, fig = gr.check_launch(d, orc, gr.synth_got(d, bad, probs=c.probs), probs=c.probs, atol=cr.ATOL)
    print(f"GENCTLREF {mut}: {fails[:2]}")
    assert fails, f"{mut} passes the checks of case {c.name}"


def test_mutation_list():
    assert len(cr.MUTATIONS) >= 10 and set(cr.MUTATIONS.values()) <= set(CASE)


def test_the_planter_moves_a_name_that_misses_a_guard_and_says_so():
    """top_p put on a cumulative mass of step 0 (every name starts from the same state): the planter
    moves that name's top_p to the middle of a gap and reports the name."""
    c = CASE["cb-N9"]
    d = cr.case_inputs(c)
    ctl = cr.controls(c)
    n = int(np.flatnonzero((ctl["plen"] == 0) & (ctl["top_p"] < 1) & (ctl["top_p"] > 0.1) & (ctl["inv_temp"] != 0))[0])
    run = cr._run(d, ctl, None, True)
    ctl["top_p"][n] = np.float32(run["cm"][0, n, 20])
    assert any(b["n"] == n and b["what"] == "top_p" for b in cr.clearance(ctl, cr._run(d, ctl, None, True)))
    fixed, run2 = cr.plant(d, ctl)
    assert fixed["moved"] == [n] and not cr.clearance(fixed, run2)
    assert abs(float(fixed["top_p"][n]) - float(ctl["top_p"][n])) < 0.05

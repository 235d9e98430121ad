"""CPU tests of models/gen_soft_ref.py, the reference of the persistent generator's soft launch: its case
list is the issue's, neutral soft values give gen_ctl_ref's / gen_con_ref's trajectory, its float64 rows are
cpu_ref.generate's with the same soft keywords on the same uniforms, the recorded emulator deviations
(which size the guards) reproduce, the float32 emulator alone passes every check that
tests/test_gen_persist_soft_gpu.py makes of a launch, and every planted defect (gen_soft_ref.MUTATIONS)
fails that same checker on the case named for it.  It also holds the engine test's settings
(tests/test_soft_persist_gpu.py imports them) and shows fp32 cpu_ref to stay at the project's bar on them."""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import gen_con_ref as nr
from gru_mpi_cuda_amd.models import gen_ctl_ref as cr
from gru_mpi_cuda_amd.models import gen_ref as gr
from gru_mpi_cuda_amd.models import gen_soft_ref as sr
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

CASE = {c.name: c for c in sr.SOFT_CASES}
CFG = GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10, sos=0, eos=0, seed=4)   # the GPU tests' model
BAR = 0.995            # tests/test_sampling_ctl_gpu.py's fp32-vs-fp64 bar
LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


@functools.lru_cache(maxsize=None)
def setup(name):
    return sr.case_setup(CASE[name])


def test_case_list_is_the_issue_s():
    for m in sr.MODES:
        n = [c for c in sr.CASES_N if c.mode == m]
        assert [c.ctl.N for c in n] == [1, 8, 9, 16, 17, 33] and all((c.ctl.H, c.ctl.L, c.ctl.ML) == (256, 1, 4) for c in n)
        assert {(c.ctl.H, c.ctl.L) for c in sr.CASES_A if c.mode == m} == {hl for hl in gr.VARIANTS if sr.supported(*hl, m)}
    assert {hl for hl in gr.VARIANTS if not sr.supported(*hl, "auto")} == {(1024, 2)}
    assert all(sr.supported(*hl, m) for hl in gr.VARIANTS for m in ("none", "mask"))
    assert [(c.ctl.H, c.ctl.L, c.ctl.N) for c in sr.CASES_T if c.mode == "none"] == [(1024, 2, 1), (1024, 2, 17)]
    assert all(c.ctl.N == 3 for c in sr.CASES_A) and all(c.ctl.ML in (4, 5) and c.ctl.V == 256 for c in sr.SOFT_CASES)
    g = [(c.ctl.N, (c.ctl.sos, c.ctl.eos), c.ctl.probs) for c in sr.CASES_G]
    assert set(g) == {(N, se, p) for N in (4, 20) for se in ((7, 3), (0, 0)) for p in (True, False)}
    assert len(CASE) == len(sr.SOFT_CASES)


@pytest.mark.parametrize("name", ["none-n-N17", "mask-n-N33", "auto-n-N9", "none-t-H1024-N17"])
def test_values_hold_what_can_go_wrong(name):
    c = CASE[name]
    d, ctl, con, soft, orc = setup(name)
    N, ML = c.ctl.N, c.ctl.ML
    tab = soft["tab"]
    assert not tab[0].any() and (tab * 4 == np.round(tab * 4)).all() and np.abs(tab).max() <= 4 and tab[1:].any(-1).all()
    assert soft["idx"][0] == soft["rows"] - 1 and not orc["soft_oob"].any()      # the last line is in use
    for a in (soft["pres"], soft["freq"]):
        assert (a * 4 == np.round(a * 4)).all() and np.abs(a).max() <= 4 and (a < 0).any() and (a > 0).any()
    forced = np.arange(ML)[:, None] < ctl["plen"][None, :]
    free = ~forced & (ctl["inv_temp"] != 0)[None, :]
    walked = ((soft["pres"] != 0) | (soft["freq"] != 0))[None, :]
    assert free[0].any(), "no step-0 sample (an empty history)"
    assert not orc["count"][0].any()
    # forced prefixes that hold one char twice and three times, counted at a sampled step of a penalised name
    top = orc["count"].max(-1)
    assert ((top == 2) & free & walked).any() and ((top == 3) & free & walked).any()
    reps = [n for n in range(N) if ctl["plen"][n] in (2, 3) and len(set(ctl["prefix"][n, :ctl["plen"][n]])) == 1]
    assert reps and all(orc["count"][ctl["plen"][n], n, ctl["prefix"][n, 0]] == ctl["plen"][n] for n in reps if walked[0, n])
    # the counts are those of the output row
    for t in range(ML):
        want = (orc["out"][:, :t, None] == np.arange(256)[None, None, :]).sum(1)
        assert np.array_equal(orc["count"][t], np.where(walked[0][:, None], want, 0))
    # a forced step reads none of it
    assert all(torch.equal(orc["v"][t, n], orc["logits"][t, n]) for t, n in np.argwhere(forced))


@pytest.mark.parametrize("name", [c.name for c in sr.CASES_G if c.ctl.probs])
def test_a_dead_name_counts_nuls(name):
    c = CASE[name]
    d, ctl, con, soft, orc = setup(name)
    assert not orc["alive_after"][1].any()
    walked = (soft["pres"] != 0) | (soft["freq"] != 0)
    even = [n for n in range(0, c.ctl.N, 2) if walked[n]]
    assert even
    for n in even:      # sampled while dead at the last step: NULs after the row's end, the EOS byte itself when eos = 0
        row = orc["out"][n]
        end = int(np.flatnonzero(row[:c.ctl.ML] == c.ctl.eos)[0])
        nul = (c.ctl.ML - 1) - (end + 1) + (1 if c.ctl.eos == 0 else 0)
        assert orc["count"][c.ctl.ML - 1, n, 0] == nul + int((row[:end] == 0).sum()) > 0


def test_the_extreme_lines_sit_on_one_char_names_only():
    c = sr.CASES_X[0]
    d, ctl, con, soft, orc = setup(c.name)
    big = np.abs(soft["tab"]).max(-1) == sr.BIG
    assert big.sum() == 2 and big[soft["idx"][0] if ctl["inv_temp"][0] == 0 else soft["idx"]].any()
    one = (ctl["inv_temp"] == 0) | (ctl["top_k"] == 1)
    assert one.any() and (big[soft["idx"]] == one).all() and soft["idx"].max() == soft["rows"] - 1
    for t, n in np.argwhere((np.arange(c.ctl.ML)[:, None] >= ctl["plen"][None, :]) & one[None, :]):
        assert orc["keep"][t, n].sum() == 1 and orc["sampled"][t, n] == (77, 200)[soft["idx"][n] - (sr.LINES - 2)]


@pytest.mark.parametrize("c", sr.CASES_F, ids=lambda c: c.name)
def test_neutral_values_give_the_trajectory_without_them(c):
    d, ctl, con, soft, orc = setup(c.name)
    if con is None:
        plain_ctl, plain = cr.plant(d, sr.controls(c))
        emus = cr.emulate(d, plain_ctl, plain["rf"]), sr.emulate(d, ctl, con, soft, orc["rf"])
    else:
        plain_ctl, plain = nr.plant(d, sr.controls(c), con)
        emus = nr.emulate(d, plain_ctl, con, plain["rf"]), sr.emulate(d, ctl, con, soft, orc["rf"])
    assert np.array_equal(plain["rf"], orc["rf"])
    for a, b in ((plain, orc), emus):
        for k, v in a.items():
            x, y = (z.numpy() if torch.is_tensor(z) else np.asarray(z) for z in (v, b[k]))
            assert np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("name", ["none-n-N16", "none-n-N17", "none-n-N33", "none-x-extreme-N12", "none-b-pen-N12",
                                  "none-b-bias-N33", "none-t-H1024-N17"])
def test_rows_equal_cpu_ref_generate_on_fp64_parameters(name):
    """The same model as cpu_ref parameters (an identity embedding behind W_ih0 = P^T, b_ih0 = 0), the same
    uniforms, controls and soft values: cpu_ref.generate's rows are the reference's."""
    c = CASE[name]
    k = c.ctl
    d, ctl, con, soft, run = setup(name)
    w = d["w64"]
    cfg = GRUConfig(vocab=k.V, embed=k.V, hidden=k.H, layers=k.L, max_len=k.ML, sos=k.sos, eos=k.eos)
    params = {"embedding": torch.eye(k.V, dtype=torch.float64), "weight_ih_l0": w["P"].T.contiguous(),
              "bias_ih_l0": torch.zeros(3 * k.H, dtype=torch.float64), "fc.weight": w["Wfc"], "fc.bias": w["bfc"]}
    for l in range(k.L):
        params[f"weight_hh_l{l}"], params[f"bias_hh_l{l}"] = w["Whh"][l], w["bhh"][l]
        if l:
            params[f"weight_ih_l{l}"], params[f"bias_ih_l{l}"] = w["Wih"][l], w["bih"][l]
    inv = ctl["inv_temp"].astype(np.float64)
    T = np.where(inv == 0, 0.0, 1.0 / np.where(inv == 0, 1.0, inv))          # 0.5, 1, 2: exact both ways
    pre = np.full((k.N, k.ML + 1), k.eos, np.uint8)               # encode_names rows: the chars, then the EOS byte
    for n in range(k.N):
        pre[n, :ctl["plen"][n]] = ctl["prefix"][n, :ctl["plen"][n]]
    rows = cpu_ref.generate(params, cfg, run["rf"].reshape(-1), temperature=T, top_k=ctl["top_k"], top_p=ctl["top_p"], prefix=pre,
                            soft=sr.as_cpu_ref(soft))
    assert np.array_equal(rows, run["out"])


@pytest.fixture(scope="module")
def measured():
    return sr.measure_deviations()


def test_recorded_deviations_reproduce(measured):
    """MEASURED_DEV is what ``python -m gru_mpi_cuda_amd.models.gen_soft_ref`` prints, rounded up to three
    digits; the guards are 8 x and the tolerances 4 x those figures."""
    for k, v in sr.MEASURED_DEV.items():
        print(f"GENSOFTREF {k}: measured {measured[k]:.3e}, recorded {v:.3e}")
        assert measured[k] <= v <= 1.01 * measured[k] + 1e-12, k
    assert sr.GUARD_Y == 8 * sr.MEASURED_DEV["y"] and sr.GUARD_MASS == max(1e-4, 8 * sr.MEASURED_DEV["mass"])
    assert sr.ATOL["probs"] == 4 * sr.MEASURED_DEV["probs"] and all(sr.ATOL[k] == gr.ATOL[k] for k in gr.ATOL if k != "probs")


@pytest.mark.parametrize("c", sr.SOFT_CASES, ids=lambda c: c.name)
def test_emulator_passes_the_launch_checker(c):
    d, ctl, con, soft, orc = setup(c.name)                        # plant asserts the guards and the cap on moved names
    assert not sr.clearance(ctl, orc) and len(ctl["moved"]) <= max(c.ctl.N // 8, 1)
    emu = sr.emulate(d, ctl, con, soft, orc["rf"])
    assert np.array_equal(emu["out"], orc["out"]) and np.array_equal(emu["sampled"], orc["sampled"])
    assert np.array_equal(emu["state_after"], orc["state_after"]) and np.array_equal(emu["count"], orc["count"])
    got = gr.synth_got(d, emu, par=len(c.name) % 2, probs=c.ctl.probs)
    fails, fig = gr.check_launch(d, orc, got, probs=c.ctl.probs, atol=sr.ATOL)
    assert not fails, fails


def _checked(c, d, orc, run):
    return gr.check_launch(d, orc, gr.synth_got(d, run, probs=c.ctl.probs), probs=c.ctl.probs, atol=sr.ATOL)


@pytest.mark.parametrize("mut", sorted(sr.MUTATIONS))
def test_every_mutation_fails_the_launch_checker(mut):
    c = CASE[sr.MUTATIONS[mut]]
    d, ctl, con, soft, orc = setup(c.name)
    fails, _ = _checked(c, d, orc, sr.emulate(d, ctl, con, soft, orc["rf"]))
    assert not fails, fails
    fails, fig = _checked(c, d, orc, sr.emulate(d, ctl, con, soft, orc["rf"], mut))
    print(f"GENSOFTREF {mut}: {fails[:2]}")
    assert fails, f"{mut} passes the checks of case {c.name}"


@pytest.mark.parametrize("mut", sorted(sr.INVISIBLE))
def test_a_reordered_rounding_is_inside_the_tolerances(mut):
    """The one defect of the issue's list that no output of a launch can show (gen_soft_ref's docstring): the
    adjusted logits differ in their last bits, and every row, id, state and probability the checker reads
    does not, beyond the tolerances.  (tests/test_gen_persist_soft_gpu.py pins the order by byte-identity
    with the per-char sampler.)"""
    c = CASE[sr.INVISIBLE[mut]]
    d, ctl, con, soft, orc = setup(c.name)
    good = sr.emulate(d, ctl, con, soft, orc["rf"])
    bad = sr.emulate(d, ctl, con, soft, orc["rf"], mut)
    free = torch.from_numpy(orc["sampled_step"]).unsqueeze(-1)
    dv = float(((bad["v"] - good["v"]).abs() * free).max())
    print(f"GENSOFTREF {mut}: largest |v - v'| on a sampled step {dv:.3e}")
    assert 0 < dv <= 2e-6
    fails, _ = _checked(c, d, orc, bad)
    assert not fails, fails


def test_mutation_list():
    assert len(sr.MUTATIONS) == 8 and len(sr.INVISIBLE) == 1 and set(sr.MUTATIONS.values()) | set(sr.INVISIBLE.values()) <= set(CASE)


# ------------------------------------------------------------------------------- the engine test's settings
def engine_cases(N):
    """What tests/test_soft_persist_gpu.py runs through HipGenerator: per-name bias lines and penalties that
    depend on the name's row AND on its batch of 64 (a batch that read rows 0.. would show), alone, with
    per-position constraints and with a regex; each with the sampling controls of the bench."""
    i = np.arange(N)
    soft = dict(logit_bias=[{chr(97 + (n + 3 * (n // 64)) % 26): 2.0, "xqz": -1.0, 0: -0.25 * (n % 5)} for n in range(N)],
                presence_penalty=0.25 * ((i + i // 64) % 4), frequency_penalty=0.5 * (i % 3))
    ctl = dict(top_k=40, top_p=0.95, temperature=0.8)
    return {
        "alone": dict(soft, **ctl),
        "pattern": dict(soft, **ctl, constraints=dict(pattern="[A-Z][a-z]", charset=LETTERS, min_len=3)),
        "regex": dict(soft, **ctl, constraints=dict(regex="[A-Z][a-z]+(son|sen)?", max_len=8)),
    }


ENGINE_N = 200
ENGINE_SEEDS = {"alone": 21, "pattern": 22, "regex": 23}
_engine = {}


def engine_oracle(case):
    """(uniforms, fp64 rows) of an engine case, computed once."""
    if case not in _engine:
        rf = random_floats(ENGINE_N, CFG.max_len, seed=ENGINE_SEEDS[case])
        p64 = {k: v.double() for k, v in init_params(CFG).items()}
        _engine[case] = (rf, cpu_ref.generate(p64, CFG, rf, **engine_cases(ENGINE_N)[case]))
    return _engine[case]


@pytest.mark.parametrize("case", sorted(ENGINE_SEEDS))
def test_fp32_cpu_ref_stays_at_the_bar_on_the_engine_test_s_settings(case):
    """The reference alone is within the cap before any GPU run: fp32 cpu_ref against the fp64 oracle."""
    rf, want = engine_oracle(case)
    got = cpu_ref.generate(init_params(CFG), CFG, rf, **engine_cases(ENGINE_N)[case])
    s = float((got == want).all(1).mean())
    print(f"GENSOFTREF engine {case}: fp32 cpu_ref names identical to the fp64 oracle: {s}")
    assert s >= BAR
    soft = cpu_ref.make_soft(CFG, ENGINE_N, *(engine_cases(ENGINE_N)[case][k] for k in ("logit_bias", "presence_penalty", "frequency_penalty")))
    assert len({(soft.idx[n], soft.presence[n], soft.frequency[n]) for n in range(64)} ^
               {(soft.idx[n], soft.presence[n], soft.frequency[n]) for n in range(64, 128)}) > 0

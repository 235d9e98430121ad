"""The beam search's reference module (models/beam_ref.py) and CPU rule (cpu_ref.beam_search): the
oracle against brute force and against ``score``, the emulator against the checker, the planted
defects, the planter, and the condition the GPU test relies on (at most one prefix in eight unsettled)."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import beam_ref as br
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params


def p64(p):
    return {k: v.double() for k, v in p.items()}


# ------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("eos", [0, 5])
def test_oracle_equals_brute_force(eos):
    """V = 64, max_len = 2: every possible output row scored (fp64), the best 32 and the best one."""
    cfg = GRUConfig(vocab=64, embed=16, hidden=16, layers=2, max_len=2, sos=0, eos=eos, seed=3)
    p = init_params(cfg)
    p["fc.weight"] = p["fc.weight"] * 64
    rows = [(eos, 0, 0)] + [(a, b, 0) for a in range(64) if a != eos for b in range(64)]
    rows = np.array(rows, np.uint8)
    lp = cpu_ref.score(p64(p), cfg, rows)[1]
    order = np.lexsort((np.arange(len(rows)), -lp))
    lp0 = torch.log_softmax(cpu_ref.forward(p64(p), cfg, torch.tensor([[cfg.sos]]))[0, 0], -1).numpy()
    first = np.lexsort((np.arange(64), -lp0))      # the first chars, best first
    for W in (32, 1):
        res = cpu_ref.beam_search(p64(p), cfg, [""], W)
        orc = br.oracle(p, cfg, [""], W)
        assert np.array_equal(res.rows, orc["rows"]) and np.abs(res.logp - orc["logp"]).max() < 1e-12
        # what a beam of W returns at max_len = 2: the best W of the rows whose first char is among the W
        # best first chars.  At W = 32 on this model those are the best 32 of ALL rows.
        kept = set(first[:W].tolist())
        best = [i for i in order if int(rows[i, 0]) in kept][:W]
        if W == 32:
            assert best == order[:W].tolist()
        assert np.array_equal(res.rows[0], rows[best])
        assert np.abs(res.logp[0] - lp[best]).max() < 1e-12
        assert res.n_beams[0] == W


def test_oracle_logp_is_the_score_of_its_rows():
    for c in br.TRAJ_CASES:
        if c.V != 64 or c.W not in (3, 32) or c.ML != 6:
            continue
        cfg, p = br.case_model(c)
        orc = br.case_oracle(c)
        s64 = br.score64_of(p, cfg, orc)
        for n in range(len(c.prefixes)):
            nb = int(orc["n_beams"][n])
            assert np.abs(orc["logp"][n, :nb] - s64[n, :nb]).max() < 1e-12, (c.name, n)
        res = cpu_ref.beam_search(p64(p), cfg, list(c.prefixes), c.W)
        for k in ("rows", "n_tok", "n_beams"):
            assert np.array_equal(getattr(res, k), orc[k]), (c.name, k)
        fin = np.isfinite(orc["logp"])
        assert np.array_equal(np.isfinite(res.logp), fin) and np.abs(res.logp[fin] - orc["logp"][fin]).max() < 1e-12
        assert br.check_result(cfg, c.prefixes, orc, res, s64) == []


def test_beam_inputs_validation():
    cfg = GRUConfig(vocab=64, embed=16, hidden=16, layers=1, max_len=4, sos=0, eos=5)
    for kw in (dict(width=0), dict(width=33), dict(width=2.5), dict(prefix="0" + chr(5)), dict(prefix="01234"),
               dict(prefix="A"), dict(prefix=["0", "1"], count=3)):
        with pytest.raises(ValueError):
            cpu_ref.beam_inputs(cfg, **kw)
    with pytest.raises(ValueError):
        cpu_ref.beam_inputs(cfg.replace(vocab=16), None, 17)
    with pytest.raises(ValueError):
        cpu_ref.beam_inputs(cfg.replace(max_len=65), None, 2)
    rows, plen = cpu_ref.beam_inputs(cfg, None, 4, count=3)
    assert rows.shape == (3, 4) and (plen == 0).all()
    rows, plen = cpu_ref.beam_inputs(cfg, "01", 4)
    assert rows.shape == (1, 4) and plen[0] == 2
    res = cpu_ref.beam_search(init_params(cfg), cfg, ["0123", ""], 3)
    assert res.names()[0] == ["0123"] and len(res.names()[1]) == 3 and res.logp.dtype == np.float32


# ------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("i", range(0, len(br.STEP_CASES), 2))
def test_emulator_passes_and_planter_clears(i):
    c = br.STEP_CASES[i]
    d = br.plant_step(br.step_inputs(c, i % 3))
    ref = br.select_ref(d)
    assert (ref["clear"] >= br.GUARD).all()
    assert len(d["moved"]) <= max(c.N // 8, 1)
    assert br.check_step(ref, br.select_emulate(d)) == []


def test_planter_moves_at_most_one_name_in_eight():
    moved = total = 0
    for i, c in enumerate(br.STEP_CASES):
        d = br.plant_step(br.step_inputs(c, i % 3))
        moved += len(d["moved"])
        total += c.N
    assert moved * 8 <= total, (moved, total)


def test_planter_clears_a_thin_gap():
    c = br.StepCase(64, 2, 1, 1, False, "free", "live", 5)
    d = br.step_inputs(c, 0)
    # beam 1's best candidate 2e-5 above beam 0's best (a planted exact tie of three): inside the guard
    lp = br.select_ref(d)["lp"]
    d["score"][1] = np.float32(d["score"][0] + lp[0].max() - lp[1].max() + 2e-5)
    assert br.select_ref(d)["clear"][0] < br.GUARD
    d2 = br.plant_step(d)
    assert d2["moved"] == [0] and br.select_ref(d2)["clear"][0] >= br.GUARD


STEP_MUTS = [m for m, (kind, _) in br.MUTATIONS.items() if kind == "step"]


@pytest.mark.parametrize("mut", STEP_MUTS)
def test_step_mutation_is_caught(mut):
    cases = [(i, c) for i, c in enumerate(br.STEP_CASES) if br.mutation_applies(mut, c)]
    assert cases, mut
    caught = 0
    for i, c in cases:
        d = br.plant_step(br.step_inputs(c, i % 3))
        caught += bool(br.check_step(br.select_ref(d), br.select_emulate(d, mut)))
    # a case may leave a defect invisible (no finished beam near the top, say); most must show it
    assert caught * 2 > len(cases), (mut, caught, len(cases))


@pytest.mark.parametrize("mut", [m for m, (kind, _) in br.MUTATIONS.items() if kind == "traj"])
def test_trajectory_mutation_is_caught(mut):
    c = next(x for x in br.TRAJ_CASES if x.name == br.MUTATIONS[mut][1])
    cfg, p = br.case_model(c)
    orc = br.case_oracle(c)
    good = br.emulate(p, cfg, c.prefixes, c.W)
    assert br.check_result(cfg, c.prefixes, orc, good, br.score64_of(p, cfg, good)) == []
    bad = br.emulate(p, cfg, c.prefixes, c.W, mut)
    assert br.check_result(cfg, c.prefixes, orc, bad, br.score64_of(p, cfg, bad)) != []


def test_mutation_list_is_complete():
    assert set(br.MUTATIONS) >= {"ties_descending_j", "carry_dropped", "finished_extended", "forced_unrestricted",
                                 "forced_lp_not_added", "pre_step_h", "row_wrong_parent", "late_bias_skipped", "unsorted",
                                 "dead_offered"}


# ------------------------------------------------------------------------------- the GPU test's condition
@pytest.mark.parametrize("c", br.TRAJ_CASES, ids=lambda c: c.name)
def test_at_most_one_prefix_in_eight_is_unsettled(c):
    """A condition, not a measurement: tests/test_beam_gpu.py compares bytes on settled prefixes only."""
    orc = br.case_oracle(c)
    unsettled = int((~orc["settled"]).sum())
    assert unsettled * 8 <= len(c.prefixes), (c.name, unsettled, orc["clear"].min(1))
    kinds = {min(len(s), 3) if len(s) < c.ML else "full" for s in c.prefixes}
    assert "full" in kinds and (c.name == "m-W32" or 0 in kinds)      # empty, short and full-length prefixes in one call


def test_guard_and_tolerances_follow_the_measured_deviations():
    assert br.GUARD == 8.0 * br.MEASURED_DEV["cand"]
    assert br.ATOL["logp"] == 4.0 * br.MEASURED_DEV["logp"] and br.ATOL["cand"] == 4.0 * br.MEASURED_DEV["cand"]
    # the written figures are the measurement's: steps in full, the trajectories of the largest model
    dev = {k: 0.0 for k in br.MEASURED_DEV}
    for i, c in enumerate(br.STEP_CASES):
        for seed in (0, 1, 2):
            for k, v in br.step_deviation(c, seed).items():
                dev[k] = max(dev[k], v)
    for c in br.TRAJ_CASES:
        for k, v in br.traj_deviation(c).items():
            if k in dev:
                dev[k] = max(dev[k], v)
    for k in dev:
        assert dev[k] <= br.MEASURED_DEV[k] and dev[k] > 0.8 * br.MEASURED_DEV[k], (k, dev[k])

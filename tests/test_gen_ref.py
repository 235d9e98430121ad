"""CPU tests of models/gen_ref.py: the guard of every planted uniform and the recorded emulator
deviations reproduce, the emulator alone passes every check that tests/test_gen_gpu.py makes of a
persistent launch, the workspace decoder inverts its encoder and matches the kernel's address
formulas, every planted defect (gen_ref.MUTATIONS) fails that same checker, and the gates / scorer
references agree with cpu_ref on a small model."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import gen_ref as gr
from gru_mpi_cuda_amd.models.params import init_params

CASE = {c.name: c for c in gr.PERSIST_CASES}


@pytest.fixture(scope="module")
def measured():
    """Every GPU case at seeds 0, 1, 2 through the oracle and the emulator.  plant_uniforms asserts the
    guard of each uniform as it places it, and measure_deviations that the emulator's sampled ids and
    output rows are the oracle's."""
    return gr.measure_deviations(seeds=(0, 1, 2))


def test_recorded_deviations_cover_the_measured_ones(measured):
    for k, v in gr.MEASURED_DEV.items():
        print(f"GENREF {k:10s} measured {measured[k]:.3e} recorded {v:.3e}")
        assert 0 < measured[k] <= v, k
        assert v <= 1.5 * measured[k] + 1e-12, f"{k}: the recorded figure is not the measured one"
        assert gr.ATOL[k] == 4.0 * v and gr.RTOL[k] == 0.0


def test_guard_is_no_thinner_than_the_arithmetic_it_protects(measured):
    assert gr.GUARD == max(1e-5, 8.0 * gr.MEASURED_DEV["cdf"])
    assert gr.GUARD >= 8.0 * measured["cdf"]


def test_case_list_is_the_issue_s():
    assert {(c.H, c.L) for c in gr.CASES_A} == set(gr.VARIANTS) and all(c.N == 3 for c in gr.CASES_A)
    assert [c.N for c in gr.CASES_B] == [1, 2, 8, 9, 16, 17, 32, 33, 48, 49, 64]
    assert [c.N for c in gr.CASES_C] == [1, 8, 9, 16, 17, 64]
    assert sorted({c.ML for c in gr.CASES_F}) == [1, 2, 10] and {c.V for c in gr.CASES_E} == {512}
    assert [c.N for c in gr.CASES_H] == [16, 5, 64, 8]
    custom = sum(1 for c in gr.PERSIST_CASES if (c.sos, c.eos) == (7, 3))
    assert 2 * custom >= len(gr.PERSIST_CASES)
    assert len({c.name for c in gr.PERSIST_CASES}) == len(gr.PERSIST_CASES)


@pytest.mark.parametrize("c", gr.PERSIST_CASES, ids=lambda c: c.name)
def test_emulator_passes_the_launch_checker(c):
    """The reference alone meets every condition the GPU test imposes: the float32 emulator's states,
    logits, ids, rows and probabilities, encoded as a launch leaves them, pass check_launch."""
    d = gr.case_inputs(c)
    orc = gr.plant_uniforms(d, gr.case_plan(c))
    assert np.abs(gr.oracle(d, orc["rf"])["states"].numpy() - orc["states"].numpy()).max() == 0   # oracle re-runs the plan
    emu = gr.emulate(d, orc["rf"])
    assert np.array_equal(emu["out"], orc["out"]) and np.array_equal(emu["sampled"], orc["sampled"])
    fails, fig = gr.check_launch(d, orc, gr.synth_got(d, emu, par=len(c.name) % 2, probs=c.probs), probs=c.probs)
    assert not fails, fails
    if c.plan == "ends01":
        assert not orc["alive_after"][0, 0] and orc["alive_after"][0, 1] and not orc["alive_after"][1, 1]
        assert orc["alive_after"][-1, 2:].all() and orc["out"][0, 0] == c.eos and not orc["out"][0, 1:].any()
    if c.plan == "all_end":
        assert not orc["alive_after"][1].any()
        assert gr.chars_run(orc["alive_after"], c.ML, c.probs) == (c.ML if c.probs else 2)


@pytest.mark.parametrize("mut", sorted(gr.MUTATIONS))
def test_every_mutation_fails_the_launch_checker(mut):
    c = CASE[gr.MUTATIONS[mut]]
    d = gr.case_inputs(c)
    orc = gr.plant_uniforms(d, gr.case_plan(c))
    bad = gr.emulate(d, orc["rf"], mut)
    fails, fig = gr.check_launch(d, orc, gr.synth_got(d, bad, probs=c.probs), probs=c.probs)
    print(f"GENREF {mut}: {fails[:2]}")
    assert fails, f"{mut} passes the checks of case {c.name}"


def test_mutation_list():
    assert len(gr.MUTATIONS) >= 10 and set(gr.MUTATIONS.values()) <= set(CASE)


@pytest.mark.parametrize("H,L,V,ML,N,T", [(1024, 2, 256, 3, 5, 3), (1024, 1, 256, 3, 8, 2), (1024, 2, 256, 3, 9, 3),
                                          (256, 2, 512, 4, 3, 4), (512, 1, 256, 4, 20, 2), (256, 3, 256, 2, 64, 2)])
def test_ws_decode_inverts_ws_encode(H, L, V, ML, N, T):
    rng = np.random.default_rng(H + N)
    sf = gr.set_floats(H, L, V, ML)
    base = rng.integers(0, 2 ** 32, 2 * sf, dtype=np.uint32)
    st = rng.standard_normal((L, ML, N, H)).astype(np.float32)
    lg = rng.standard_normal((ML, N, V)).astype(np.float32)
    ids = rng.integers(0, 2 ** 17, (ML, N)).astype(np.uint32)
    for par in (0, 1):
        ws = gr.ws_encode(base, par, st, lg, ids, H, L, V, ML, N, T)
        dec = gr.ws_decode(ws, par, H, L, V, ML, N, T)
        assert np.array_equal(dec["states"][:, :T], st[:, :T]) and np.array_equal(dec["logits"][:T], lg[:T])
        if N > 16:
            k = min(T, ML - 1)
            assert np.array_equal(dec["ids"][:k], ids[:k])
        own = dec["mask"]
        s = slice(par * sf, (par + 1) * sf)
        assert np.array_equal(ws[s][~own], base[s][~own])            # the encoder writes owned slots only
        # the kernel's address formulas (gen_persist.hip: xoff, xoffp, lg0, id0), in words of the set
        f = ws[s].view(np.float32)
        l, t, n, h = L - 1, T - 1, N - 1, H - 3
        if gr.tagged_states(H, N):
            a = ((l * ML + t) * 256 + h // 4) * 32 + n * 4 + h % 4
        else:
            a = ((l * ML + t) * 64 + n) * H + h
        assert f[a] == st[l, t, n, h] and own[a]
        lg0 = L * ML * 64 * H
        assert f[lg0 + (t * 64 + n) * V + V - 2] == lg[t, n, V - 2] and own[lg0 + (t * 64 + n) * V + V - 2]
        id0 = lg0 + ML * 64 * V
        assert own[id0 + n] == (N > 16 and min(T, ML - 1) > 0)
        assert not own[id0 + (ML - 1) * 64 + n]                       # the last char's id is never published
        if T < ML:
            assert not own[lg0 + (T * 64) * V] and not own[((0 * ML + T) * 64) * H if not gr.tagged_states(H, N) else (T * 256) * 32]
        nw = gr.rows_written(N)
        if nw < 64:
            assert not own[lg0 + nw * V]
        # the other set: refilled
        o = ws[(1 - par) * sf:(2 - par) * sf]
        rs, rl = gr.refill_floats(H, L, V, ML)
        assert (o[:rs] == gr.EMPTY).all() and (o[lg0:lg0 + rl] == gr.EMPTY).all()
        assert np.array_equal(o[rs:lg0], base[(1 - par) * sf:(2 - par) * sf][rs:lg0])


def test_checker_sees_a_write_outside_the_owned_slots():
    c = CASE["g-N4-all-end-early-exit"]
    d = gr.case_inputs(c)
    orc = gr.plant_uniforms(d, gr.case_plan(c))
    emu = gr.emulate(d, orc["rf"])
    ok = gr.synth_got(d, emu, probs=False)
    assert not gr.check_launch(d, orc, ok, probs=False)[0]
    late = gr.synth_got(d, emu, probs=False, T=c.ML)                  # no early exit: chars >= 2 written
    assert any("outside the launch's slots" in f for f in gr.check_launch(d, orc, late, probs=False)[0])
    for key, i in (("sync", 3), ("err", 0)):
        g = dict(ok)
        g[key] = ok[key].copy()
        g[key][i] = 32
        assert gr.check_launch(d, orc, g, probs=False)[0]
    g = dict(ok)
    g["out"] = ok["out"].copy()
    g["out"][c.N, 0] = 0
    assert gr.check_launch(d, orc, g, probs=False)[0]


# ------------------------------------------------------------------------------ gates / scorer vs cpu_ref
def test_gates_and_scorer_references_agree_with_cpu_ref():
    cfg = GRUConfig(vocab=64, embed=16, hidden=24, layers=2, max_len=6, sos=5, eos=2)
    params = {k: v.double() for k, v in init_params(cfg, seed=3).items()}
    rng = np.random.default_rng(0)
    rows = rng.integers(0, cfg.vocab, (7, cfg.max_len + 1)).astype(np.uint8)
    rows[0, 0] = cfg.eos
    rows[1, 3] = cfg.eos
    rows[2, cfg.max_len - 1] = cfg.eos
    rows[3][rows[3] == cfg.eos] = 9
    Bp, ML, V, H = 8, cfg.max_len, cfg.vocab, cfg.hidden
    ids, tgt, ntok, bad = gr.score_prep_ref(rows, 7, Bp, ML, V, cfg.sos, cfg.eos)
    _, n_tok, x, t = cpu_ref.score_inputs(cfg, rows)
    assert not bad and np.array_equal(ntok[:7], n_tok) and ntok[7] == 0
    assert np.array_equal(ids[:, :7].T, x) and np.array_equal(tgt[:, :7].T, t)
    assert (ids[:, 7] == cfg.sos).all() and (tgt[:, 7] == -1).all()
    # the model through gates_ref, one step at a time
    inp = params["embedding"][torch.from_numpy(ids.T.astype(np.int64))]          # [Bp][ML][E]
    for l in range(cfg.layers):
        Wih, Whh = params[f"weight_ih_l{l}"], params[f"weight_hh_l{l}"]
        bih, bhh = params[f"bias_ih_l{l}"], params[f"bias_hh_l{l}"]
        h = torch.zeros(Bp, H, dtype=torch.float64)
        outs = []
        for s in range(ML):
            d = dict(Bp=Bp, H=H, V=V, table=False, Gh=(h @ Whh.T).reshape(1, -1), Gi=(inp[:, s] @ Wih.T).reshape(1, -1),
                     bgh=bhh, bgi=bih, hprev=h)
            h = gr.gates_ref(d)
            outs.append(h)
        inp = torch.stack(outs, 1)
    logits = inp @ params["fc.weight"].T + params["fc.bias"]                       # [Bp][ML][V]
    ref_logits = cpu_ref.forward(params, cfg, torch.from_numpy(x))
    assert float((logits[:7] - ref_logits).abs().max()) < 1e-12
    d = dict(V=V, ML=ML, Bp=Bp, splits=1, slab=0, logits=logits.permute(1, 0, 2).reshape(1, -1), bias=None,
             tgt=torch.from_numpy(tgt), ntok=torch.from_numpy(ntok))
    lp, name, rank, nt = gr.score_ref(d)
    rlp, rname, rnt, rrank = cpu_ref.score(params, cfg, rows)
    assert np.abs(lp.numpy()[:7] - rlp).max() < 1e-12 and np.abs(name.numpy()[:7] - rname).max() < 1e-12
    assert np.array_equal(rank.numpy()[:7], rrank) and np.array_equal(nt.numpy()[:7], rnt)
    assert float(name[7]) == 0 and (rank[7] == -1).all()


def test_score_prep_ref_clamps_and_flags_a_byte_outside_the_vocabulary():
    rows = np.array([[70, 1, 2, 0], [1, 2, 70, 0]], np.uint8)       # eos = 2: row 1's 70 lies after its EOS
    ids, tgt, ntok, bad = gr.score_prep_ref(rows, 2, 2, 3, 64, 5, 2)
    assert bad and tgt[0, 0] == 0 and ids[1, 0] == 0 and list(ntok) == [3, 2] and tgt[2, 1] == -1
    assert not gr.score_prep_ref(rows[1:], 1, 1, 3, 64, 5, 2)[3]


def test_planted_scorer_inputs_hold_what_they_claim():
    for a in gr.SCORE_CASES:
        d = gr.score_inputs(*a)
        lp, name, rank, nt = gr.score_ref(d)
        V, ML, Bp = a[0], a[1], a[2]
        assert {0, 1, ML} <= set(nt.tolist())
        seen = set()
        for b in range(Bp):
            for l in range(int(nt[b])):
                k = (l + b) % 6
                seen.add(k)
                t = int(d["tgt"][l, b])
                if k == 1:
                    assert rank[b, l] == 0
                elif k == 2:
                    assert rank[b, l] == V - 1
                elif k == 4:
                    assert rank[b, l] == t                            # all equal: the lower indices come first
        if ML >= 6:
            assert seen == set(range(6))
        assert bool(torch.isfinite(lp).all()) and bool(torch.isnan(d["logits"]).any())


def test_hsplit_of_is_the_bf16_split():
    h = torch.tensor([[1.0, 0.3, -0.7123, 1e-3]])
    w = gr.hsplit_of(h)
    hi = (w[:, :4] << 16).to(torch.int32).view(torch.float32)
    lo = (w[:, 8:] << 16).to(torch.int32).view(torch.float32)
    assert torch.equal(w[:, :4], w[:, 4:8]) and float((hi + lo - h).abs().max()) < 2 ** -16

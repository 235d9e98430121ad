"""Soft sampling preferences on the CPU (docs/DESIGN.md §4h): cpu_ref.make_soft and the logit bias,
presence and frequency penalties in cpu_ref.generate / score / filter_probs."""
import itertools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

CFG = GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10, sos=0, eos=0, seed=4)   # the GPU tests' model
BAR = 0.995            # tests/test_sampling_ctl_gpu.py's fp32-vs-fp64 bar
SMALL = GRUConfig(vocab=64, embed=16, hidden=32, layers=1, max_len=6, sos=0, eos=0, seed=2)
_cache = {}


def model(cfg=CFG):
    key = (cfg.vocab, cfg.hidden, cfg.max_len)
    if key not in _cache:
        _cache[key] = init_params(cfg)
    return _cache[key]


def f64(p):
    return {k: v.double() for k, v in p.items()}


# The soft settings the GPU tests run through HipGenerator (tests/test_soft_ctl_gpu.py imports them, with
# the seeds): multiples of 0.25 are not needed here -- the model's logits are not planted.
def soft_cases(N):
    i = np.arange(N)
    return {
        "alone": dict(logit_bias={"xqz": -2.0, 0: -1.0, "ae": 0.5}, presence_penalty=0.75, frequency_penalty=0.5),
        "sampled": dict(logit_bias={"aeiou": 1.0, 0: -0.5}, presence_penalty=0.5, frequency_penalty=0.25,
                        top_k=20, top_p=0.9, temperature=0.8),
        "prefix": dict(logit_bias={0: -1.5}, frequency_penalty=1.0, prefix=[("Mar", "", "J", "Ka")[n % 4] for n in range(N)]),
        "pattern": dict(logit_bias={"abc": 1.5}, presence_penalty=1.0,
                        constraints=dict(pattern="[A-Z][a-z]", charset="abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")),
        "regex": dict(logit_bias={"n": 1.0, 0: 0.5}, presence_penalty=0.5, frequency_penalty=0.5,
                      constraints=dict(regex="[A-Z][a-z]+(son|sen)?", max_len=8)),
        # per-name values: name i's depend on i and on its batch of 64
        "per_name": dict(logit_bias=[{chr(97 + (n + n // 64) % 26): 2.0, 0: -0.25 * (n % 5)} for n in range(N)],
                         presence_penalty=0.25 * ((i + i // 64) % 4), frequency_penalty=0.5 * (i % 3)),
    }


SEEDS = {"alone": 9, "sampled": 9, "prefix": 10, "pattern": 11, "regex": 12, "per_name": 13}


# ------------------------------------------------------------------------------- make_soft
def test_make_soft_builds_a_table_with_line_zero_and_distinct_lines():
    s = cpu_ref.make_soft(CFG, 5, [{"ab": 1.0}, None, {"a": 1.0, "b": 1.0}, np.zeros(256), {97: 0.5, "a": 0.5, b"b": 1}],
                          0.5, [0, 1, 2, 3, 4])
    assert s.tab.dtype == np.float32 and s.tab.shape == (2, 256) and (s.tab[0] == 0).all()
    assert s.idx.tolist() == [1, 0, 1, 0, 1] and s.tab[1, 97] == 1 and s.tab[1, 98] == 1 and s.tab[1].sum() == 2
    assert s.presence.tolist() == [0.5] * 5 and s.frequency.tolist() == [0, 1, 2, 3, 4]
    one = cpu_ref.make_soft(CFG, 3, np.arange(256) / 256)
    assert one.idx.tolist() == [1, 1, 1] and one.rows == 2
    part = s.slice(2, 2)
    assert part.tab is s.tab and part.idx.tolist() == [1, 0] and part.frequency.tolist() == [2, 3]
    assert cpu_ref.make_soft(CFG, 0).idx.shape == (0,)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1.0001e4, -2e4])
def test_make_soft_rejects_non_finite_and_huge_values(bad):
    for kw in (dict(logit_bias={"a": bad}), dict(logit_bias=np.full(256, bad)), dict(presence_penalty=bad),
               dict(frequency_penalty=[0.0, bad, 0.0]), dict(logit_bias=[None, {"a": 1}, {5: bad}])):
        with pytest.raises(ValueError):
            cpu_ref.make_soft(CFG, 3, **kw)
    cpu_ref.make_soft(CFG, 3, {"a": 1e4, "b": -1e4}, 1e4, -1e4)   # the bound itself is fine


def test_make_soft_rejects_wrong_lengths_keys_and_too_many_lines():
    with pytest.raises(ValueError):
        cpu_ref.make_soft(CFG, 3, presence_penalty=[1.0, 2.0])
    with pytest.raises(ValueError):
        cpu_ref.make_soft(CFG, 3, frequency_penalty=np.zeros(4))
    with pytest.raises(ValueError):
        cpu_ref.make_soft(CFG, 3, logit_bias=[{"a": 1}, {"b": 1}])          # two rows for three names
    with pytest.raises(ValueError):
        cpu_ref.make_soft(CFG, 3, logit_bias=np.zeros(255))
    with pytest.raises(ValueError):
        cpu_ref.make_soft(CFG, 3, logit_bias=np.zeros((3, 255)))
    small = CFG.replace(vocab=64)
    for key in ("a", 64, -1, b"\xff", "Ā", 1.5):
        with pytest.raises(ValueError):
            cpu_ref.make_soft(small, 3, logit_bias={key: 1.0})
    cpu_ref.make_soft(small, 3, logit_bias={"0": 1.0, 63: 1.0})
    rows = [{7: 0.25 * (n + 1)} for n in range(256)]                         # 256 distinct lines + line 0
    with pytest.raises(ValueError):
        cpu_ref.make_soft(CFG, 256, logit_bias=rows)
    assert cpu_ref.make_soft(CFG, 255, logit_bias=rows[:255]).rows == 256


def test_make_soft_penalties_need_a_byte_vocabulary():
    big = CFG.replace(vocab=512)
    for kw in (dict(presence_penalty=0.5), dict(frequency_penalty=[0.0, 0.0, 0.25])):
        with pytest.raises(ValueError):
            cpu_ref.make_soft(big, 3, **kw)
    s = cpu_ref.make_soft(big, 3, {300: 1.0}, 0.0, 0.0)                      # a bias alone is fine, neutral penalties too
    assert s.tab.shape == (2, 512) and s.tab[1, 300] == 1
    with pytest.raises(ValueError):
        cpu_ref.generate(model(), CFG, random_floats(2, 10, seed=1), soft=s)             # a Soft of another vocabulary
    with pytest.raises(ValueError):
        cpu_ref.generate(model(), CFG, random_floats(2, 10, seed=1), soft=cpu_ref.make_soft(CFG, 2), logit_bias={"a": 1})


# ------------------------------------------------------------------------------- the rule
def test_soft_adjust_is_the_three_operations_in_order():
    """fp32: (x + b) - (f * n (+ p if n > 0)), each rounded; values chosen so that another order differs."""
    V = 64
    cfg = GRUConfig(vocab=V)
    x = torch.tensor([[1e8] + [0.1] * (V - 1)], dtype=torch.float32)
    s = cpu_ref.make_soft(cfg, 1, {0: 3.0, 1: 1.0}, presence_penalty=3.0, frequency_penalty=0.1)
    em = np.array([[0, 0, 1]], np.uint8)
    v = cpu_ref.soft_adjust(x, s, em)
    f32 = np.float32
    pen0 = f32(f32(0.1) * f32(2)) + f32(3.0)
    assert v[0, 0].item() == f32(f32(f32(1e8) + f32(3.0)) - f32(pen0))       # 1e8 + 3 rounds to 1e8: not x + (b - pen)
    assert v[0, 1].item() == f32(f32(f32(0.1) + f32(1.0)) - f32(f32(f32(0.1) * f32(1)) + f32(3.0)))
    assert v[0, 2].item() == f32(0.1)                                        # no occurrence: no presence term
    assert (cpu_ref.soft_adjust(x, s, None)[0, 2:] == x[0, 2:]).all()
    # the counts ignore bytes outside the vocabulary
    assert (cpu_ref.soft_adjust(x, s, np.array([[200, 255, 64]], np.uint8)) == cpu_ref.soft_adjust(x, s, None)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_neutral_soft_controls_are_the_call_without_them(dtype):
    p = {k: v.to(dtype) for k, v in model().items()}
    N = 48
    rf = random_floats(N, CFG.max_len, seed=5)
    zero = dict(logit_bias=np.zeros(256), presence_penalty=0.0, frequency_penalty=np.zeros(N))
    for ctl in (dict(), dict(top_k=20, top_p=0.9, temperature=0.8), dict(prefix="Jo", constraints=dict(regex="[A-Za-z]+"))):
        want = cpu_ref.generate(p, CFG, rf, **ctl)
        assert (cpu_ref.generate(p, CFG, rf, **ctl, **zero) == want).all()
        assert (cpu_ref.generate(p, CFG, rf, **ctl, logit_bias={}) == want).all()
        assert (cpu_ref.generate(p, CFG, rf, **ctl, soft=cpu_ref.make_soft(CFG, N)) == want).all()
        a = cpu_ref.score(p, CFG, want, **ctl, **zero)
        b = cpu_ref.score(p, CFG, want, **ctl)
        assert len(a) == 5                                                   # the controlled rule: n_kept comes back
        for u, v in zip(a, b):
            assert (u.view(np.uint8) == v.view(np.uint8)).all()


def test_a_huge_bias_forces_or_bans_a_char():
    p = model()
    N = 40
    rf = random_floats(N, CFG.max_len, seed=6)
    rows = cpu_ref.generate(p, CFG, rf, logit_bias={"q": 1e4}, prefix="Ab")
    assert (rows[:, :2] == np.frombuffer(b"Ab", np.uint8)).all() and (rows[:, 2:CFG.max_len] == ord("q")).all()
    plain = cpu_ref.generate(p, CFG, rf)
    common = np.bincount(plain[:, :3].reshape(-1), minlength=256)[1:].argmax() + 1   # a char the model does emit
    assert (plain == common).any()
    rows = cpu_ref.generate(p, CFG, rf, logit_bias={int(common): -1e4})
    assert not (rows[:, :CFG.max_len] == common).any()
    # -1e4 on EOS: every name runs to max_len
    rows = cpu_ref.generate(p, CFG, rf, logit_bias={CFG.eos: -1e4})
    assert (rows[:, :CFG.max_len] != CFG.eos).all()


def test_a_huge_frequency_penalty_leaves_no_repeated_char():
    p = model()
    N = 60
    rf = random_floats(N, CFG.max_len, seed=7)
    noeos = {CFG.eos: -1e4}                                                  # full-length names: ten chars to repeat among
    plain = cpu_ref.generate(p, CFG, rf, logit_bias=noeos, top_k=5)
    assert any(len(set(r[:CFG.max_len])) < CFG.max_len for r in plain)       # the setting does repeat without it
    for kw in (dict(frequency_penalty=1e4), dict(presence_penalty=1e4)):
        rows = cpu_ref.generate(p, CFG, rf, logit_bias=noeos, top_k=5, **kw)
        assert all(len(set(r[:CFG.max_len])) == CFG.max_len for r in rows)
    # forced prefix chars count: after "aa" no further a
    rows = cpu_ref.generate(p, CFG, rf, logit_bias={"a": 5.0, CFG.eos: -1e4}, frequency_penalty=1e4, prefix="aa")
    assert (rows[:, :2] == ord("a")).all() and not (rows[:, 2:CFG.max_len] == ord("a")).any()


def test_an_eos_bias_moves_the_mean_length():
    p = model()
    N = 200
    rf = random_floats(N, CFG.max_len, seed=8)

    def mean_len(**kw):
        return float(cpu_ref.score_inputs(CFG, cpu_ref.generate(p, CFG, rf, **kw))[1].mean())

    base, longer, shorter = mean_len(), mean_len(logit_bias={CFG.eos: -3.0}), mean_len(logit_bias={CFG.eos: 3.0})
    print("mean n_tok: eos bias -3:", longer, "none:", base, "+3:", shorter)
    assert shorter < base < longer


def test_score_sums_to_one_over_all_rows_of_a_tiny_model():
    """vocab = 64, max_len = 3: every distinct output row (a char != EOS continues, EOS stops, three chars
    are a full row) scored in fp64 under soft controls with a charset and a top-k: the probabilities sum to 1
    within 1e-9, and the rows the sampler cannot emit are exactly -inf."""
    cfg = GRUConfig(vocab=64, embed=16, hidden=32, layers=1, max_len=3, sos=0, eos=0, seed=3)
    p = f64(init_params(cfg))
    chars = range(1, 64)
    names = [()] + [(a,) for a in chars] + [(a, b) for a in chars for b in chars]
    rows = np.zeros((len(names) + 63 ** 3, 4), np.uint8)
    for i, nm in enumerate(names):
        rows[i, :len(nm)] = nm
    rows[len(names):, :3] = np.array(list(itertools.product(chars, repeat=3)), np.uint8)
    N = rows.shape[0]
    cs = bytes(range(33, 59))
    soft = dict(logit_bias={bytes([40, 41]): 1.5, 0: -0.75, 50: -2.0}, presence_penalty=1.25, frequency_penalty=0.5)
    for ctl in (dict(), dict(constraints=dict(charset=cs)), dict(constraints=dict(charset=cs), top_k=7, top_p=0.9, temperature=0.7)):
        tok, name, n_tok, rank, n_kept = cpu_ref.score(p, cfg, rows, **soft, **ctl)
        total = float(np.exp(name).sum())
        print(sorted(ctl), "sum of exp(name_logp):", total, "impossible rows:", int(np.isneginf(name).sum()))
        assert abs(total - 1.0) <= 1e-9
        if "constraints" in ctl:
            inside = np.isin(rows[:, :3], np.frombuffer(cs, np.uint8)) | (rows[:, :3] == 0)
            assert np.isneginf(name[~inside.all(1)]).all()
        if "top_k" in ctl:
            live = np.arange(3)[None, :] < n_tok[:, None]
            assert (n_kept[live] <= ctl["top_k"]).all() and np.isneginf(name).any()
    # and the soft terms do change the distribution
    assert not np.array_equal(cpu_ref.score(p, cfg, rows[:200], **soft)[1], cpu_ref.score(p, cfg, rows[:200])[1])


def test_score_is_the_log_probability_of_what_generate_emits():
    """Rows generated with soft controls are possible under them, step by step inside the kept set; scoring
    them under other soft values gives other numbers."""
    p = f64(model(SMALL))
    N = 64
    rf = random_floats(N, SMALL.max_len, seed=3)
    kw = dict(logit_bias={5: 2.0, 0: -1.0}, presence_penalty=1.0, frequency_penalty=0.5, top_k=6, top_p=0.9, prefix=[b"\x07"] * N)
    rows = cpu_ref.generate(p, SMALL, rf, **kw)
    tok, name, n_tok, rank, n_kept = cpu_ref.score(p, SMALL, rows, **kw)
    assert np.isfinite(name).all()
    live = np.arange(SMALL.max_len)[None, :] < n_tok[:, None]
    assert (n_kept[live] >= 1).all() and (n_kept[live] <= 6).all() and (n_kept[:, 0] == 1).all()
    assert (rank == cpu_ref.score(p, SMALL, rows)[3]).all()                  # rank stays the model's
    other = cpu_ref.score(p, SMALL, rows, **dict(kw, frequency_penalty=2.0))[1]
    assert not np.array_equal(other, name)


@pytest.mark.parametrize("case", list(SEEDS))
def test_fp32_reference_stays_inside_the_bar_with_soft_controls(case):
    """The share of names on which fp32 cpu_ref.generate equals the fp64 oracle, for the settings and seeds of
    tests/test_soft_ctl_gpu.py at N = 70: the reference's own arithmetic reaches the bar."""
    N = 70
    rf = random_floats(N, CFG.max_len, seed=SEEDS[case])
    kw = soft_cases(N)[case]
    a = cpu_ref.generate(model(), CFG, rf, **kw)
    b = cpu_ref.generate(f64(model()), CFG, rf, **kw)
    share = float((a == b).all(1).mean())
    print(case, "fp32 names identical to the fp64 oracle:", share)
    assert share >= BAR
    assert not (b == cpu_ref.generate(f64(model()), CFG, rf, **{k: v for k, v in kw.items() if k not in
                                                                  ("logit_bias", "presence_penalty", "frequency_penalty")})).all()

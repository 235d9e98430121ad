"""Constrained names on the CPU (docs/DESIGN.md §4e): the pattern parser and the table, and the rule
inside cpu_ref.generate, cpu_ref.beam_search and filter_probs."""
import itertools
import string

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

CFG = GRUConfig(vocab=256, embed=16, hidden=24, layers=2, max_len=8, sos=0, eos=0, seed=3)
LETTERS = string.ascii_letters


def sets_of(c, n=0):
    """Name n's allowed chars per step, as sorted byte strings."""
    a = c.allowed()[n]
    return [bytes(np.flatnonzero(a[l]).astype(np.uint8)) for l in range(a.shape[0])]


# ------------------------------------------------------------------------------- parser and table
def test_pattern_items_classes_ranges_negation_escapes_and_dot():
    c = cpu_ref.make_constraints(CFG, 1, pattern=r"M[aeiou].[a-c][^a-y]\.\[[x\]\-]", charset="abcxyz.")
    s = sets_of(c)
    assert s[0] == b"M"                      # a literal stands for itself, inside charset or not
    assert s[1] == b"aeiou"
    assert s[2] == b".abcxyz"                # . = any char of charset
    assert s[3] == b"abc"
    assert s[4] == b".z"                     # a negated class is taken inside charset
    assert s[5] == b"." and s[6] == b"["     # escapes
    assert s[7] == b"-]x"                    # escaped ] and - inside a class
    assert c.tab.dtype == np.uint32 and c.tab.shape[1] == CFG.vocab // 32 and c.idx.dtype == np.int32
    # P items imply min_len >= P: no EOS before step P (here P = max_len, so never)
    assert all(CFG.eos not in x for x in s)


def test_lengths_and_positions_past_the_pattern():
    c = cpu_ref.make_constraints(CFG, 1, pattern="Ma", charset=LETTERS, min_len=4, max_len=6)
    s = sets_of(c)
    letters = bytes(sorted(LETTERS.encode()))
    assert s[0] == b"M" and s[1] == b"a"
    assert s[2] == letters and s[3] == letters               # past the pattern: charset, no EOS before min_len
    assert s[4] == b"\0" + letters and s[5] == b"\0" + letters
    assert s[6] == b"\0"                                     # step max_len: only EOS
    assert len(s[7]) == CFG.vocab                            # never reached: no constraint
    full = sets_of(cpu_ref.make_constraints(CFG, 1, max_len=CFG.max_len, min_len=CFG.max_len))
    assert all(len(x) == CFG.vocab - 1 and 0 not in x for x in full)     # exactly max_len chars: EOS nowhere


def test_table_is_deduplicated_with_line_zero_all_ones():
    c = cpu_ref.make_constraints(CFG, 4, pattern=["ab", "ab", None, "[ab]b"], charset=[LETTERS, LETTERS, None, LETTERS])
    assert (c.tab[0] == 0xFFFFFFFF).all()
    assert len({r.tobytes() for r in c.tab}) == c.rows       # distinct lines
    assert (c.idx[0] == c.idx[1]).all()
    assert (c.idx[2] == 0).all()                             # a free name among constrained ones: line 0
    assert c.idx[0, 1] == c.idx[3, 1] and c.idx[0, 0] != c.idx[3, 0]
    assert c.idx[0, 2] == c.idx[3, 2] != 0
    none = cpu_ref.make_constraints(CFG, 3)
    assert none.rows == 1 and (none.idx == 0).all() and (none.tab == 0xFFFFFFFF).all()
    # bit c % 32 of word c / 32
    one = cpu_ref.make_constraints(CFG, 1, pattern="A")
    line = one.tab[one.idx[0, 0]]
    assert line[65 // 32] == 1 << (65 % 32) and (np.delete(line, 65 // 32) == 0).all()


def test_per_name_values_and_slices():
    c = cpu_ref.make_constraints(CFG, 3, charset=LETTERS, min_len=[1, 2, 3], max_len=5)
    for n in range(3):
        s = sets_of(c, n)
        assert [0 in x for x in s[:6]] == [l >= n + 1 for l in range(6)]
    assert (c.slice(1, 2).idx == c.idx[1:3]).all() and c.slice(1, 2).tab is c.tab
    with pytest.raises(ValueError):
        cpu_ref.make_constraints(CFG, 3, min_len=[1, 2])


@pytest.mark.parametrize("kw", [
    dict(min_len=5, max_len=3),                      # an empty set at step 3
    dict(charset="", min_len=1),                     # nothing to write at step 0
    dict(pattern="[^a]", charset="a"),               # a negated class that leaves nothing
    dict(pattern="[Ā]"), dict(pattern="é"), dict(charset="é"),      # (vocab 128 below) a byte >= vocab
    dict(pattern="[ab"), dict(pattern="ab]"), dict(pattern="ab\\"), dict(pattern="[]"), dict(pattern="[z-a]"),
    dict(pattern="a" * 9),                           # longer than max_len
    dict(pattern="abc", max_len=2),                  # the pattern does not fit under max_len
    dict(max_len=9), dict(min_len=-1),
])
def test_bad_constraints_raise(kw):
    cfg = CFG.replace(vocab=128)
    with pytest.raises(ValueError):
        cpu_ref.make_constraints(cfg, 2, **kw)


def test_too_many_distinct_sets_raise():
    cfg = GRUConfig(vocab=256, embed=8, hidden=8, layers=1, max_len=8, seed=1)
    pats = ["[%s]" % "".join(chr(65 + j) for j in range(12) if (i >> j) & 1 or j == 11) for i in range(1100)]
    with pytest.raises(ValueError):
        cpu_ref.make_constraints(cfg, len(pats), pattern=pats)


def test_prefix_outside_its_set_raises():
    p = init_params(CFG)
    rf = random_floats(2, CFG.max_len, seed=1)
    with pytest.raises(ValueError):
        cpu_ref.generate(p, CFG, rf, prefix="Mx", constraints=dict(pattern="M[aeiou]"))
    with pytest.raises(ValueError):
        cpu_ref.beam_search(p, CFG, "Mx", 2, constraints=dict(pattern="M[aeiou]"))
    with pytest.raises(ValueError):
        cpu_ref.generate(p, CFG, rf, prefix="Mari", constraints=dict(max_len=3))     # only EOS at step 3
    cpu_ref.generate(p, CFG, rf, prefix="Ma", constraints=dict(pattern="M[aeiou]"))


# ------------------------------------------------------------------------------- generate
def obeys(row, sets, eos=0):
    """A row stays inside its per-step sets up to and including its EOS."""
    for l, ch in enumerate(row[:len(sets)]):
        if ch not in sets[l]:
            return False
        if ch == eos:
            return True
    return True


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_generate_obeys_pattern_charset_and_lengths(dt):
    p = {k: v.to(dt) for k, v in init_params(CFG).items()}
    N = 60
    rf = random_floats(N, CFG.max_len, seed=5)
    kw = dict(pattern=["M[aeiou].", "[A-Z][a-z]", None] * 20, charset=[LETTERS, LETTERS + "-", None] * 20,
              min_len=[4, 2, None] * 20, max_len=[7, 3, None] * 20)
    cons = cpu_ref.make_constraints(CFG, N, **kw)
    got = cpu_ref.generate(p, CFG, rf, constraints=cons)
    assert (got == cpu_ref.generate(p, CFG, rf, constraints=kw)).all()       # the dict form
    for n in range(N):
        assert obeys(got[n], sets_of(cons, n)), n
    names = [bytes(r).split(b"\0")[0].decode("latin-1") for r in got]
    for nm in names[0::3]:
        assert 4 <= len(nm) <= 7 and nm[0] == "M" and nm[1] in "aeiou" and all(c in LETTERS for c in nm)
    for nm in names[1::3]:
        assert 2 <= len(nm) <= 3 and nm[0].isupper() and nm[1].islower() and all(c in LETTERS + "-" for c in nm)
    # the free names of the mixed batch are the unconstrained ones
    plain = cpu_ref.generate(p, CFG, rf)
    assert (got[2::3] == plain[2::3]).all() and not (got[0::3] == plain[0::3]).all()
    # with sampling controls on top
    got = cpu_ref.generate(p, CFG, rf, temperature=0.7, top_k=3, top_p=0.8, constraints=cons)
    assert all(obeys(got[n], sets_of(cons, n)) for n in range(N))
    greedy = cpu_ref.generate(p, CFG, rf, temperature=0.0, constraints=cons)
    assert all(obeys(greedy[n], sets_of(cons, n)) for n in range(N))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_generate_line_zero_only_and_literal_pattern(dt):
    p = {k: v.to(dt) for k, v in init_params(CFG).items()}
    N = 40
    rf = random_floats(N, CFG.max_len, seed=6)
    free = cpu_ref.make_constraints(CFG, N)
    assert (cpu_ref.generate(p, CFG, rf, constraints=free) == cpu_ref.generate(p, CFG, rf)).all()
    ctl = dict(temperature=0.8, top_k=5, top_p=0.9)
    assert (cpu_ref.generate(p, CFG, rf, constraints=free, **ctl) == cpu_ref.generate(p, CFG, rf, **ctl)).all()
    assert (cpu_ref.generate(p, CFG, rf, constraints=dict(pattern="Mar")) == cpu_ref.generate(p, CFG, rf, prefix="Mar")).all()
    # start / count: name n keeps its uniforms and its constraint
    part = cpu_ref.generate(p, CFG, rf, 10, 5, constraints=dict(pattern="Mar"))
    assert (part == cpu_ref.generate(p, CFG, rf, prefix="Mar")[10:15]).all()


# ------------------------------------------------------------------------------- beam search
TINY = GRUConfig(vocab=3, embed=4, hidden=5, layers=1, max_len=3, sos=0, eos=0, seed=7)


def tiny_constraints(name):
    """Over the vocabulary {EOS, 1, 2}."""
    kw = {"free": {}, "only2": dict(charset="\x02"), "len2": dict(min_len=2, max_len=2),
          "1then2": dict(pattern="\x01\x02")}[name]
    return cpu_ref.make_constraints(TINY, 1, **kw)


def enumerate_rows(cfg):
    """Every output row the generator can write: chars up to an EOS, or max_len chars."""
    ML, V = cfg.max_len, cfg.vocab
    rows = set()
    for seq in itertools.product(range(V), repeat=ML):
        seq = list(seq)
        if cfg.eos in seq:
            seq = seq[:seq.index(cfg.eos) + 1]
        rows.add(bytes(seq + [0] * (ML + 1 - len(seq))))
    return sorted(rows)


@pytest.mark.parametrize("name", ["free", "only2", "len2", "1then2"])
def test_beam_search_equals_brute_force_on_a_tiny_model(name):
    """width 32 holds every candidate of a 3-char vocabulary over 3 steps, so the search is exhaustive:
    its result is every row that satisfies the constraint, ordered by fp64 log-probability."""
    p64 = {k: v.double() for k, v in init_params(TINY).items()}
    cons = tiny_constraints(name)
    sets = sets_of(cons)
    rows = np.array([np.frombuffer(r, np.uint8) for r in enumerate_rows(TINY)])
    assert len(rows) == 1 + 2 + 4 + 8
    lp = cpu_ref.score(p64, TINY, rows)[1]
    ok = np.array([obeys(r, sets) for r in rows])
    order = np.argsort(-lp[ok], kind="stable")
    want_rows, want_lp = rows[ok][order], lp[ok][order]
    assert np.diff(want_lp).max() < -1e-9                     # no ties: the order is the scores'
    # (beam_search itself refuses a width above the vocabulary, the device's limit: the rule has none)
    pre, plen = cpu_ref.beam_inputs(TINY, "", 1)
    got = cpu_ref.beam_search_rule(p64, TINY, pre, plen, 32, cons)
    nb = int(got.n_beams[0])
    assert nb == len(want_rows) == {"free": 15, "only2": 4, "len2": 4, "1then2": 3}[name]
    assert (got.rows[0, :nb] == want_rows).all()
    np.testing.assert_allclose(got.logp[0, :nb], want_lp, rtol=0, atol=1e-12)
    assert np.isneginf(got.logp[0, nb:]).all() and (got.rows[0, nb:] == 0).all()      # dead slots last
    # a narrower beam still returns only rows that satisfy the constraint, best first
    w2 = cpu_ref.beam_search(p64, TINY, "", 2, constraints=cons)
    assert all(obeys(r, sets) for r in w2.rows[0, :int(w2.n_beams[0])])


def test_beam_select_allowed_masks_live_beams_only():
    lp = np.log(np.array([[0.5, 0.3, 0.2], [0.1, 0.1, 0.8]]))
    score = np.array([-1.0, -0.5])
    state = np.array([cpu_ref.BEAM_LIVE, cpu_ref.BEAM_FIN])
    allowed = np.array([False, False, True])
    sel = cpu_ref.beam_select(lp, score, state, allowed=allowed)
    assert [(b, c) for b, c, _, _ in sel] == [(1, -1), (0, 2)]           # the carry (j = V, char 0) is not masked
    assert sel[0][2] == -0.5 and np.isclose(sel[1][2], -1.0 + np.log(0.2))
    forced = cpu_ref.beam_select(lp, score, state, forced_char=1, allowed=allowed)
    assert [(b, c) for b, c, _, _ in forced] == [(1, -1), (-1, -1)]      # a forced char outside the set: not offered
    assert cpu_ref.beam_select(lp, score, state)[0][:2] == (1, -1)


# ------------------------------------------------------------------------------- the sampling rule
def test_filter_probs_masked_argmax_small_set_and_singleton():
    x = torch.tensor([3.0, 1.0, 2.0, 0.5, 2.0, -1.0, 0.0, 1.5], dtype=torch.float64)
    V = len(x)
    A = np.array([False, True, True, False, True, False, True, False])     # the arg-max (0) is masked
    p = cpu_ref.filter_probs(x, allowed=A)
    assert (p[~torch.from_numpy(A)] == 0).all() and abs(float(p.sum()) - 1) < 1e-12
    want = torch.softmax(x[A], -1)
    assert torch.allclose(p[A], want, atol=1e-15)
    g = cpu_ref.filter_probs(x, temperature=0.0, allowed=A)
    assert g.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]                          # the lowest index of the maximum over A
    # top-k counts inside A: k = 2 keeps the tie at 2.0 (indices 2, 4); the masked 3.0 takes no slot
    k2 = cpu_ref.filter_probs(x, top_k=2, allowed=A)
    assert (k2 > 0).tolist() == [False, False, True, False, True, False, False, False]
    k3 = cpu_ref.filter_probs(x, top_k=3, allowed=A)
    assert (k3 > 0).tolist() == [False, True, True, False, True, False, False, False]
    # an allowed set smaller than k is kept whole, and nothing outside it
    k6 = cpu_ref.filter_probs(x, top_k=6, allowed=A)
    assert ((k6 > 0).numpy() == A).all() and torch.equal(k6, p)
    # a singleton
    one = np.zeros(V, bool)
    one[5] = True
    for kw in (dict(), dict(top_k=3), dict(top_p=0.5), dict(temperature=0.0), dict(temperature=2.0, top_k=1, top_p=1e-6)):
        s = cpu_ref.filter_probs(x, allowed=one, **kw)
        assert s.tolist() == [0, 0, 0, 0, 0, 1, 0, 0], kw
    # top-p over the kept set: the mass above 2.0 inside A is 0, so p -> 0 keeps the tied maxima
    pp = cpu_ref.filter_probs(x, top_p=1e-6, allowed=A)
    assert (pp > 0).tolist() == [False, False, True, False, True, False, False, False]
    # everything allowed: today's result, bitwise
    assert torch.equal(cpu_ref.filter_probs(x, top_k=3, top_p=0.9, allowed=np.ones(V, bool)),
                       cpu_ref.filter_probs(x, top_k=3, top_p=0.9))
    with pytest.raises(ValueError):
        cpu_ref.filter_probs(x, allowed=np.zeros(V, bool))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_sample_controlled_fallback_stays_inside_the_set(dt):
    rng = np.random.default_rng(2)
    N, V = 16, 64
    x = torch.from_numpy(rng.standard_normal((N, V))).to(dt)
    A = rng.random((N, V)) < 0.2
    A[:, V - 1] = False                       # the highest allowed index lies below V - 1
    A[np.arange(N), rng.integers(0, V - 1, N)] = True
    top = np.array([V - 1 - A[n, ::-1].argmax() for n in range(N)])
    r1 = torch.ones(N)                        # past every CDF
    for kw in (dict(), dict(top_k=50), dict(temperature=0.5)):
        sel = cpu_ref.sample_controlled(x, r1, allowed=A, **kw).numpy()
        assert (sel == top).all() and A[np.arange(N), sel].all(), kw
    sel = cpu_ref.sample_controlled(x, r1, top_k=2, allowed=A).numpy()      # the highest *kept* index
    assert A[np.arange(N), sel].all()
    for r in (0.0, 0.3, 0.999):
        sel = cpu_ref.sample_controlled(x, torch.full((N,), r), allowed=A).numpy()
        assert A[np.arange(N), sel].all()
    assert torch.equal(cpu_ref.sample_controlled(x, torch.full((N,), 0.4), allowed=np.ones((N, V), bool)),
                       cpu_ref.sample_controlled(x, torch.full((N,), 0.4)))


def test_distributed_slices_follow_the_global_name_index():
    """A rank's names keep their own lines, whichever form the constraints came in."""
    from gru_mpi_cuda_amd.engine.generator import _slice_constraints
    N = 10
    kw = dict(pattern=["%s." % chr(65 + n) for n in range(N)], charset=LETTERS, max_len=4)
    whole = cpu_ref.make_constraints(CFG, N, **kw)
    p = init_params(CFG)
    rf = random_floats(N, CFG.max_len, seed=2)
    want = cpu_ref.generate(p, CFG, rf, constraints=whole)
    assert [chr(r[0]) for r in want] == [chr(65 + n) for n in range(N)]
    for start, count in ((0, 4), (4, 3), (7, 3)):
        for form in (whole, kw):
            mine = _slice_constraints(CFG, form, N, start, count)
            got = cpu_ref.generate(p, CFG, rf, start, count, constraints=mine)
            assert (got == want[start:start + count]).all(), (start, type(form))
    assert _slice_constraints(CFG, None, N, 0, 4) is None
    with pytest.raises(ValueError):
        _slice_constraints(CFG, cpu_ref.make_constraints(CFG, N - 1), N, 0, 4)

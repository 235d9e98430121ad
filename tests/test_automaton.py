"""Automaton constraints on the CPU (docs/DESIGN.md §4g): the regex / exclusion compiler against Python's
``re`` as an independent judge, the tables' fixed rules, and cpu_ref.generate / beam_search / score through
``regex=`` against the same language written per position."""
import itertools
import re
import string

import numpy as np
import pytest

import test_score_ctl as tsc
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

AB = GRUConfig(vocab=128, max_len=5, sos=0, eos=0)
# every operator, nesting, {m,n}, an empty alternative, suffix and contains forms
REGEXES = ["a*b", "(a|b)*abb", "a+b?", "(ab|ba){1,2}", "a{2}", "a{2,}", "a{1,3}b", "(a|)b", ".*ab", ".*aa.*",
           "((a|b)(a|b))*", "[ab]{2,4}", "(a(b|a)?)+", "[^a]+", "a?b?a?", "(a|b(a|bb)){0,2}b?", "\\a.\\b"]
BOUNDS = [(None, None), (2, 4), (0, 3)]


def strings(alphabet, max_len):
    for L in range(max_len + 1):
        for t in itertools.product(alphabet, repeat=L):
            yield "".join(t)


def walk(aut, name, cfg, n=0):
    """Accepted by walking the tables: every char inside its state's set, then EOS allowed (or the row full)."""
    lines, q = aut.lines(), int(aut.start[n])
    for c in name.encode("latin-1"):
        if not lines[q, c]:
            return False
        q = int(aut.nxt[q, c])
    return len(name) == cfg.max_len or bool(lines[q, cfg.eos])


def reachable(aut):
    seen, todo = set(int(s) for s in aut.start), [int(s) for s in aut.start]
    lines = aut.lines()
    while todo:
        q = todo.pop()
        for c in np.flatnonzero(lines[q]):
            t = int(aut.nxt[q, c])
            if t not in seen:
                seen.add(t)
                todo.append(t)
    return sorted(seen)


def check_tables(aut, cfg):
    """The fixed rules: state 0 free, nxt[q][eos] = 0, nxt[q][c] = 0 outside tab[q], no reachable dead end."""
    lines = aut.lines()
    assert aut.tab.dtype == np.uint32 and aut.nxt.dtype == np.uint16 and aut.start.dtype == np.int32
    assert lines[0].all() and (aut.nxt[0] == 0).all()
    assert (aut.nxt[:, cfg.eos] == 0).all()
    assert (aut.nxt[~lines] == 0).all()
    assert int(aut.nxt.max()) < aut.states <= cpu_ref.AUTOMATON_MAX_STATES
    for q in reachable(aut):
        assert lines[q].any(), q


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("rx", REGEXES)
def test_compiler_agrees_with_re_fullmatch(rx, lo, hi):
    pyrx = rx.replace("\\a", "a").replace("\\b", "b")      # a backslash makes the next byte literal here
    want = {w for w in strings("ab", AB.max_len)
            if re.fullmatch(pyrx, w) and (lo or 0) <= len(w) <= (AB.max_len if hi is None else hi)}
    if not want:
        with pytest.raises(ValueError, match="no name is allowed"):
            cpu_ref.make_constraints(AB, 1, regex=rx, charset="ab", min_len=lo, max_len=hi)
        return
    aut = cpu_ref.make_constraints(AB, 1, regex=rx, charset="ab", min_len=lo, max_len=hi)
    assert isinstance(aut, cpu_ref.Automaton)
    check_tables(aut, AB)
    got = {w for w in strings("ab", AB.max_len) if walk(aut, w, AB)}
    assert got == want                                                   # tolerance 0
    # no char outside the alphabet is ever allowed, in any reachable state
    lines = aut.lines()
    others = np.ones(AB.vocab, bool)
    others[[AB.eos, ord("a"), ord("b")]] = False
    assert not lines[reachable(aut)][:, others].any() or 0 in reachable(aut)


def test_every_name_of_the_language_can_be_finished_from_every_reachable_state():
    """No dead end, the strong form: from every state reached by a legal walk some legal walk ends."""
    aut = cpu_ref.make_constraints(AB, 1, regex="(a|b)*abb|b{5}", charset="ab", min_len=3)
    lines = aut.lines()
    for w in strings("ab", AB.max_len):
        q, legal = int(aut.start[0]), True
        for c in w.encode():
            legal = legal and bool(lines[q, c])
            if not legal:
                break
            q = int(aut.nxt[q, c])
        if legal and len(w) < AB.max_len:
            rest = [t for t in strings("ab", AB.max_len - len(w)) if walk(aut, w + t, AB)]
            assert rest, w


def test_exclude_rejects_exactly_the_listed_names():
    names = ["ab", "", "abba", "bbbbb", "b", "aab", "toolongname"]
    aut = cpu_ref.make_constraints(AB, 1, exclude=names, charset="ab")
    check_tables(aut, AB)
    for w in strings("ab", AB.max_len):
        assert walk(aut, w, AB) == (w not in names), w
    # bytes and str name the same thing; an empty list excludes nothing and still gives an Automaton
    assert walk(cpu_ref.make_constraints(AB, 1, exclude=[b"ab"], charset="ab"), "ab", AB) is False
    free = cpu_ref.make_constraints(AB, 1, exclude=[], charset="ab")
    assert isinstance(free, cpu_ref.Automaton) and all(walk(free, w, AB) for w in strings("ab", 3))


def test_exclude_and_regex_together():
    names = ["ab", "aab", "bab", "bb"]
    aut = cpu_ref.make_constraints(AB, 1, regex=".*b", exclude=names, charset="ab", max_len=4)
    check_tables(aut, AB)
    for w in strings("ab", AB.max_len):
        assert walk(aut, w, AB) == (w.endswith("b") and len(w) <= 4 and w not in names), w


def test_per_name_values_share_one_table_and_free_names_sit_in_state_zero():
    aut = cpu_ref.make_constraints(AB, 5, regex=["a+", None, "b+", "a+", None], exclude=[None, None, ["bb"], None, ["a"]],
                                   charset=["ab", None, "ab", "ab", "ab"])
    check_tables(aut, AB)
    assert aut.start[1] == 0 and aut.start[0] == aut.start[3] and len({int(s) for s in aut.start}) == 4
    assert walk(aut, "aa", AB, 0) and not walk(aut, "ab", AB, 0) and walk(aut, "!?", AB, 1)
    assert walk(aut, "b", AB, 2) and not walk(aut, "bb", AB, 2) and walk(aut, "bbb", AB, 2)
    assert not walk(aut, "a", AB, 4) and walk(aut, "ab", AB, 4) and not walk(aut, "a!", AB, 4)
    part = aut.slice(2, 2)
    assert part.tab is aut.tab and part.start.tolist() == aut.start[2:4].tolist()


def test_state_merging_keeps_2000_random_names_under_the_cap():
    cfg = GRUConfig(vocab=256, max_len=10)
    rng = np.random.default_rng(5)
    names = ["".join(string.ascii_lowercase[c] for c in rng.integers(0, 26, 6)) for _ in range(2000)]
    aut = cpu_ref.make_constraints(cfg, 3, exclude=names, charset=string.ascii_lowercase)
    check_tables(aut, cfg)
    # a trie of the names has about 2000 * 4 distinct inner nodes; merged, the leaves' parents that exclude
    # the same last letters are one state, and the free tail is one state per remaining length
    nodes = len({nm[:k] for nm in names for k in range(7)})
    assert aut.states < nodes < cpu_ref.AUTOMATON_MAX_STATES
    assert not any(walk(aut, nm, cfg) for nm in names[:200])
    assert walk(aut, names[0][:5], cfg) and walk(aut, names[0] + "a", cfg) and walk(aut, "zzzzzzzzzz", cfg)


def test_states_with_equal_lines_and_successors_are_merged():
    # a{3}: one state per step, nothing to merge; (a|b){3} from two spellings is the same automaton
    one = cpu_ref.make_constraints(AB, 1, regex="(a|b){3}")
    two = cpu_ref.make_constraints(AB, 1, regex="(a|b)(b|a)[ab]|[ab]{3}")
    assert one.states == two.states == 5                 # the free state, three steps, the EOS-only state
    assert np.array_equal(one.tab, two.tab) and np.array_equal(one.nxt, two.nxt)
    # contains "aa": a counter over 5 steps x 3 phases, far below the unmerged product
    assert cpu_ref.make_constraints(AB, 1, regex=".*aa.*", charset="ab").states <= 1 + 3 * AB.max_len


def test_too_many_states_raise(monkeypatch):
    monkeypatch.setattr(cpu_ref, "AUTOMATON_MAX_STATES", 6)
    with pytest.raises(ValueError, match="automaton states"):
        cpu_ref.make_constraints(AB, 1, regex=".*aa.*", charset="ab")
    big = cpu_ref.Automaton(np.zeros((7, 4), np.uint32), np.zeros((7, 128), np.uint16), np.zeros(1, np.int32))
    with pytest.raises(ValueError):
        cpu_ref.as_constraints(AB, 1, big)


@pytest.mark.parametrize("kw,msg", [
    (dict(regex="a{6}"), "no name is allowed"),                          # longer than max_len = 5
    (dict(regex="a+", charset="b", min_len=1, exclude=["a", "aa", "aaa", "aaaa", "aaaaa"]), "no name is allowed"),
    (dict(regex="ab", min_len=3), "no name is allowed"),
    (dict(regex="a|\\\xff"), "vocab"),                                   # byte 255 >= V = 128
    (dict(regex="[a-\xff]"), "vocab"),
    (dict(exclude=["a\xff"]), "vocab"),
    (dict(regex="a\\\x00"), "EOS"),
    (dict(regex="[\x00-a]"), "EOS"),
    (dict(exclude=["a\x00b"]), "EOS"),
    (dict(regex="a", pattern="a"), "pattern"),
    (dict(exclude=["a"], pattern="a"), "pattern"),
    (dict(regex="(a"), "regex"), (dict(regex="a)"), "regex"), (dict(regex="a{2"), "regex"), (dict(regex="a{3,2}"), "regex"),
    (dict(regex="*a"), "regex"), (dict(regex="a**"), "regex"), (dict(regex="^a"), "regex"), (dict(regex="a$"), "regex"),
    (dict(regex="(?:a)"), "regex"), (dict(regex="[a"), "regex"), (dict(regex="a\\"), "regex"), (dict(regex="a{,2}"), "regex"),
    (dict(regex="a", max_len=6), "max_len"), (dict(regex="a", min_len=-1), "min_len"),
    (dict(regex=["a", "b"]), "got 2"), (dict(exclude=[["a"], ["b"], ["c"]]), "got 3"), (dict(exclude="ab"), "list"),
])
def test_bad_values_raise_value_error(kw, msg):
    with pytest.raises(ValueError, match=msg):
        cpu_ref.make_constraints(AB, 1, **kw)
    if not msg.startswith("got"):
        with pytest.raises(ValueError, match=msg):                       # single values are checked for 0 names too
            cpu_ref.make_constraints(AB, 0, **kw)


def test_a_prefix_the_automaton_rejects_raises():
    cfg, p = small()
    rf = random_floats(3, cfg.max_len, seed=1)
    for fn in (lambda **kw: cpu_ref.generate(p, cfg, rf, **kw),
               lambda **kw: cpu_ref.beam_search(p, cfg, width=2, **kw),
               lambda **kw: cpu_ref.score(p, cfg, np.zeros((1, cfg.max_len + 1), np.uint8), **kw)):
        with pytest.raises(ValueError, match="not allowed by the constraint"):
            fn(prefix="Mb", constraints=dict(regex="Ma.*"))
        with pytest.raises(ValueError, match="not allowed by the constraint"):
            fn(prefix="Max", constraints=dict(exclude=["Max"], max_len=3))     # "Max" could only stop here


# ------------------------------------------------------------------ the rule in generate / beam_search / score
LOWER, UPPER = string.ascii_lowercase, string.ascii_uppercase
CTL = dict(temperature=0.8, top_k=40, top_p=0.95)
# one language, two spellings: a capital, then 3 to 6 lower-case letters
AS_REGEX = dict(regex="[A-Z][a-z]{3,6}")
AS_PATTERN = dict(pattern="[A-Z]", charset=LOWER, min_len=4, max_len=7)


def small(max_len=8):
    cfg = GRUConfig(vocab=128, embed=16, hidden=24, layers=2, max_len=max_len, sos=0, eos=0, seed=2)
    p = init_params(cfg)
    p["fc.weight"] = p["fc.weight"] * 8
    return cfg, {k: v.double() for k, v in p.items()}


@pytest.mark.parametrize("max_len", [8, 7])              # 7: the longest name fills the row, no EOS step
def test_regex_and_pattern_spellings_give_identical_results(max_len):
    cfg, p = small(max_len)
    N = 64
    rf = random_floats(N, cfg.max_len, seed=3)
    pre = ["", "M", "Jo", "Anna"] * (N // 4)
    for ctl in ({}, CTL, dict(CTL, prefix=pre), dict(temperature=0.0)):
        a = cpu_ref.generate(p, cfg, rf, constraints=AS_REGEX, **ctl)
        b = cpu_ref.generate(p, cfg, rf, constraints=AS_PATTERN, **ctl)
        assert np.array_equal(a, b)
        names = [bytes(r[:cfg.max_len]).split(b"\0")[0].decode() for r in a]
        assert all(re.fullmatch("[A-Z][a-z]{3,6}", nm) for nm in names), names
        sa = cpu_ref.score(p, cfg, a, constraints=AS_REGEX, **ctl)
        sb = cpu_ref.score(p, cfg, a, constraints=AS_PATTERN, **ctl)
        assert len(sa) == len(sb) == 5
        for u, v in zip(sa, sb):                         # tok_logp, name_logp, n_tok, rank, n_kept
            assert np.array_equal(u, v)
        assert np.isfinite(sa[1]).all()
    for prefixes, W in (([""], 8), (["", "M", "Jo", "Anna"], 3)):
        a = cpu_ref.beam_search(p, cfg, prefixes, W, constraints=AS_REGEX)
        b = cpu_ref.beam_search(p, cfg, prefixes, W, constraints=AS_PATTERN)
        assert np.array_equal(a.rows, b.rows) and np.array_equal(a.logp, b.logp)
        assert np.array_equal(a.n_tok, b.n_tok) and np.array_equal(a.n_beams, b.n_beams)
        assert all(re.fullmatch("[A-Z][a-z]{3,6}", nm) for row in a.names() for nm in row)


def test_generate_suffix_contains_and_exclusion_in_one_batch():
    cfg, p = small()
    N = 48
    rf = random_floats(N, cfg.max_len, seed=5)
    kinds = [".*son", ".*ann.*", "Ma[rl][a-z]{2,4}", None]
    ex = [None, None, ["Marab", "Malab"], ["", "a"]]
    kw = dict(regex=[kinds[n % 4] for n in range(N)], exclude=[ex[n % 4] for n in range(N)],
              charset=[LOWER if n % 4 < 2 else None for n in range(N)])
    rows = cpu_ref.generate(p, cfg, rf, constraints=kw, **CTL)
    names = [bytes(r[:cfg.max_len]).split(b"\0")[0].decode("latin-1") for r in rows]
    for n, nm in enumerate(names):
        if kinds[n % 4] is not None:
            assert re.fullmatch(kinds[n % 4], nm), (n, nm)
        assert nm not in (ex[n % 4] or []), (n, nm)
    assert {len(nm) for nm in names[0::4]} != {3}        # ".*son" is not just "son"
    # the free names draw what they draw without any constraint but their tiny exclusion list
    plain = cpu_ref.generate(p, cfg, rf, **CTL)
    keep = [n for n in range(3, N, 4) if bytes(plain[n, :cfg.max_len]).split(b"\0")[0] not in (b"", b"a")]
    assert keep and np.array_equal(rows[keep], plain[keep])
    # beam: the most probable names that end in "son", exhaustive order checked by their scores
    res = cpu_ref.beam_search(p, cfg, ["", "J"], 4, constraints=dict(regex=".*son", charset=LOWER + "J"))
    assert all(nm.endswith("son") for row in res.names() for nm in row) and all(nm.startswith("J") for nm in res.names()[1])
    sc = cpu_ref.score(p, cfg, res.rows.reshape(-1, cfg.max_len + 1))[1].reshape(2, 4)
    assert np.allclose(sc, res.logp, rtol=0, atol=1e-12) and (np.diff(res.logp, axis=1) <= 0).all()


def test_score_outside_the_language_is_minus_infinity_and_later_steps_use_line_zero():
    cfg, p = small()
    from gru_mpi_cuda_amd.engine.generator import encode_names
    rows = encode_names(["Maria", "maria", "Mar", "Mariaxyz", "Ma9ia"], cfg)
    tok, name, n_tok, rank, nk = cpu_ref.score(p, cfg, rows, constraints=AS_REGEX)
    assert np.isfinite(name[0]) and np.isneginf(name[1:]).all() and not np.isnan(tok).any()
    assert np.isneginf(tok[1, 0]) and np.isfinite(tok[1, 1:6]).all()      # after the bad char: line 0, finite steps
    assert (nk[1, 1:6] == cfg.vocab).all() and nk[1, 0] == 26 and nk[0, 1] == 26 and nk[0, 4] == 27
    assert np.isneginf(tok[2, 3]) and np.isfinite(tok[2, :3]).all()       # EOS after 3 chars: too short
    assert np.isneginf(tok[3, 7]) and np.isfinite(tok[3, :7]).all()       # an eighth char
    plain = cpu_ref.score(p, cfg, rows)
    assert np.array_equal(tok[1, 1:6], plain[0][1, 1:6])


def test_probabilities_sum_to_one_over_the_language():
    """tests/test_score_ctl.py's sum-to-one test with a regex: all 4033 distinct rows of a 64-char, two-step
    model; the rows of the language carry all the mass, every other row exactly none."""
    cfg, p = tsc.small_model(0)
    rows = tsc.all_rows_ml2(0)
    rx = b"[\x08-\x17]|[\x10-\x27][^\x09]"                # one char of 8..23, or one of 16..39 and any but 9
    cs = "".join(chr(c) for c in range(8, 40))
    tok, name, n_tok, rank, nk = cpu_ref.score(p, cfg, rows, temperature=0.7, top_k=20, top_p=0.9,
                                               constraints=dict(regex=rx, charset=cs))
    inside = np.array([re.fullmatch(rx, bytes(r[:2]).split(b"\0")[0]) is not None for r in rows])
    assert 0 < inside.sum() < len(rows)
    assert not np.isnan(tok).any() and np.isneginf(name[~inside]).all()
    assert abs(np.exp(name[inside]).sum() - 1.0) <= 1e-12
    assert abs(np.exp(name).sum() - 1.0) <= 1e-12


def test_for_rows_renumbers_the_lines_it_uses():
    cfg = GRUConfig(vocab=256, max_len=10)
    rng = np.random.default_rng(2)
    names = ["".join(LOWER[c] for c in rng.integers(0, 26, 4)) for _ in range(3000)]
    aut = cpu_ref.make_constraints(cfg, 4, exclude=names, charset=LOWER)
    from gru_mpi_cuda_amd.engine.generator import encode_names
    rows = encode_names([names[0], names[1][:3], "zz", names[2] + "q"], cfg)
    cons = aut.for_rows(cfg, rows)
    assert isinstance(cons, cpu_ref.Constraints) and cons.rows <= 1 + 4 * 6 and cons.idx.shape == (4, 10)
    a = cons.allowed()
    assert not a[0, 4, cfg.eos] and a[1, 3, cfg.eos] and a[3, 5, cfg.eos]
    assert cpu_ref.as_constraints(cfg, 4, cons) is cons

"""Automaton constraints on the device (docs/DESIGN.md §4g): the AUTO instantiations of sample_ctl_f32 and
beam_select_f32 on planted inputs -- the masks' arithmetic is §4e's, so the helpers, tolerances and
clearances are those of tests/test_constraints_gpu.py; what is new and checked exactly is the state buffer
-- and HipGenerator.generate / beam_search / score with ``regex`` / ``exclude`` against the fp64 oracles,
Python's ``re`` and the same language written per position."""
import re
import string

import numpy as np
import pytest
import torch

import test_constraints_gpu as cg
import test_sampling_ctl_gpu as sc
import test_score_ctl as tsc
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import beam_ref as br
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.utils.data import random_floats

gpu = pytest.mark.gpu
DEV = "cuda"
ML, STEP, EOS = sc.ML, sc.STEP, sc.EOS
LETTERS, LOWER = string.ascii_letters, string.ascii_lowercase
t, stream, pack = cg.t, cg.stream, cg.pack
CANARY = 0x5A5A5A5A


# ------------------------------------------------------------------------------- sample_ctl_f32
S_BIG = 3000


def big_table(V, sets, seed):
    """3000 states: line 0 all ones, the rows' sets planted at random lines (the last line among them),
    every other line a random half; nxt random in [0, 3000) with the fixed zeros of the rule left out on
    purpose -- the kernel must store whatever the table says."""
    rng = np.random.default_rng(seed)
    lines = rng.random((S_BIG, V)) < 0.5
    lines[0] = True
    where = rng.choice(np.arange(1, S_BIG - 1), len(sets), replace=False)
    where[len(sets) // 2] = S_BIG - 1
    lines[where] = sets
    nxt = rng.integers(0, S_BIG, (S_BIG, V)).astype(np.uint16)
    return pack(lines), nxt, where.astype(np.int32)


def launch_auto(ext, buf, bias, R, V, slabs, r, ctl, tab, nxt, state, row0=0, alive=None, rows=None):
    """cg.launch with a state buffer in place of idx: [canary, row0 + R states, canary]."""
    lg = t(buf)
    rf = np.zeros((R, ML), np.float32)
    rf[:, STEP] = r
    rf = t(rf)
    ids = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((R, ML + 1), 7, dtype=torch.uint8, device=DEV)
    al = t(np.ones(R, np.int32) if alive is None else alive.astype(np.int32))
    probs = torch.full((R, V), -1.0, device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    cd = [t(a) for a in ctl]
    assert state.shape == (row0 + R,)
    sb = t(np.concatenate([[CANARY], state, [CANARY]]).astype(np.int32))
    dt, dn = t(tab.view(np.int32)), t(nxt.view(np.int16))
    d = dict(logits=lg.data_ptr(), splits=slabs, slab=R * V, rf=rf.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(),
             alive=al.data_ptr(), N=R, V=V, step=STEP, max_len=ML, eos=EOS, probs=probs.data_ptr(),
             inv_temp=cd[0].data_ptr(), top_k=cd[1].data_ptr(), top_p=cd[2].data_ptr(), plen=cd[3].data_ptr(),
             prefix=cd[4].data_ptr(), row0=row0, err=err.data_ptr(), allow_tab=dt.data_ptr(), allow_next=dn.data_ptr(),
             allow_state=sb.data_ptr() + 4, allow_rows=tab.shape[0] if rows is None else rows)
    if bias is not None:
        b = t(bias)
        d["bias"] = b.data_ptr()
    ext.sample_ctl(d, stream())
    torch.cuda.synchronize()
    return (ids.cpu().numpy(), out.cpu().numpy(), al.cpu().numpy(), probs.cpu().numpy(), err.cpu().numpy(),
            sb.cpu().numpy())


@gpu
@pytest.mark.parametrize("slabs,late_bias", [(1, False), (2, True)])
@pytest.mark.parametrize("V,R", [(256, 70), (512, 70), (256, 3)])
def test_sample_ctl_automaton_mask_choice_and_state_advance(ext, V, R, slabs, late_bias):
    """cg's kinds of mask x (k, p, T) per row, the line taken from the state buffer: kept set, probabilities
    and choice as in §4e, and the buffer afterwards exactly nxt[state][chosen] -- on forced rows (which read
    no mask), greedy rows, sampled rows and finished rows alike -- with the rows before row0 and the words
    around the buffer untouched."""
    x, buf, bias = sc.make_logits(V, R, slabs, late_bias, seed=3 * V + 5 * R + slabs)
    x64 = torch.from_numpy(x).double()
    rng = np.random.default_rng(V + R + slabs)
    cells = [(kd, c) for kd in cg.KINDS for c in cg.CTLS]
    for j in range(-(-len(cells) // R) if R > 3 else 4):
        mine = [cells[(j * R + i) % len(cells)] for i in range(R)]
        A = np.stack([cg.mask_of(m[0], x[i], rng) for i, m in enumerate(mine)])
        k = np.array([m[1][0] for m in mine], np.int32)
        T = np.array([m[1][2] for m in mine], np.float64)
        p = cg.clear_top_p(x64, T, k, np.array([m[1][1] for m in mine], np.float32), A)
        ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, T, k, p)
        forced = (np.arange(R) + j) % 9 == 8
        plen = np.where(forced, STEP + 1, np.arange(R) % (STEP + 1)).astype(np.int32)
        pre = ((np.arange(R)[:, None] * 7 + np.arange(ML)[None, :] * 3 + j) % V).astype(np.uint8)
        alive = (np.arange(R) + j) % 4 != 3
        want = cpu_ref.filter_probs(x64, T, k, p, allowed=A).numpy()
        want[forced] = np.eye(V)[pre[forced, STEP]]
        r = rng.random(R, dtype=np.float32)
        r[(np.arange(R) + j) % 3 == 2] = 1.5
        r, sel = sc.clear_uniforms(want, r)
        assert (T == 0).any() or R <= 3
        row0 = 5 if j % 2 else 0
        tab, nxt, line = big_table(V, A, seed=j + V)
        assert (line == S_BIG - 1).any()
        state = np.concatenate([np.full(row0, 77, np.int32), line])
        arrs = sc.pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), row0)
        ids, out, al, probs, err, sb = launch_auto(ext, buf, bias, R, V, slabs, r, arrs, tab, nxt, state, row0, alive)
        assert err[0] == 0
        free = ~forced
        assert (probs[free][~A[free]] == 0).all()
        assert ((probs > 0) == (want > 0)).all()
        torch.testing.assert_close(torch.from_numpy(probs).double(), torch.from_numpy(want), atol=2e-7, rtol=1e-5)
        assert (ids == sel).all(), (j, np.argwhere(ids != sel)[:4])
        assert (out[:, STEP] == np.where(alive, sel & 255, 7)).all() and (al == (alive & (sel != EOS))).all()
        # the state buffer, exactly
        assert sb[0] == CANARY and sb[-1] == CANARY and (sb[1:1 + row0] == 77).all()
        assert (sb[1 + row0:-1] == nxt[line, sel].astype(np.int32)).all()


@gpu
@pytest.mark.parametrize("V", [256, 512])
def test_sample_ctl_automaton_flags_a_state_outside_the_table(ext, V):
    R = 3
    x, buf, bias = sc.make_logits(V, R, 1, False, seed=1)
    rng = np.random.default_rng(0)
    A = np.stack([cg.mask_of("below_k", x[i], rng) for i in range(R)])
    tab, nxt, line = big_table(V, A, seed=4)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, 1.0, 0, 1.0)
    arrs = (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)
    r = np.full(R, 0.5, np.float32)
    for bad in (S_BIG, -1, 1 << 20):
        state = line.copy()
        state[1] = bad
        ids, _, _, probs, err, sb = launch_auto(ext, buf, bias, R, V, 1, r, arrs, tab, nxt, state)
        assert err[0] == 16 and err[1] == np.int32(bad) and err[2] == 1 and err[3] == 0
        ok = line.copy()
        ok[1] = 0                                                        # ... and the row takes line 0
        ids0, _, _, probs0, err0, sb0 = launch_auto(ext, buf, bias, R, V, 1, r, arrs, tab, nxt, ok)
        assert err0[0] == 0 and (ids == ids0).all() and (probs.view(np.uint32) == probs0.view(np.uint32)).all()
        assert (probs[1] > 0).all() and (probs[0] > 0).sum() == 3
        assert (sb == sb0).all() and sb[2] == nxt[0, ids[1]] and sb[0] == CANARY and sb[-1] == CANARY
    # allow_rows is the bound, not the buffer: the last line in use lies outside a table cut short
    _, _, _, _, err, _ = launch_auto(ext, buf, bias, R, V, 1, r, arrs, tab, nxt, line, rows=int(line.max()))
    assert err[0] == 16 and err[1] == line.max()
    # a forced row advances too, and also flags a bad state
    plen = np.full(R, STEP + 1, np.int32)
    pre = np.full((R, ML), 9, np.uint8)
    state = line.copy()
    state[2] = S_BIG + 5
    ids, _, _, _, err, sb = launch_auto(ext, buf, bias, R, V, 1, r, (ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), tab, nxt, state)
    assert (ids == 9).all() and err[0] == 16 and err[2] == 2
    assert sb[1] == nxt[line[0], 9] and sb[2] == nxt[line[1], 9] and sb[3] == nxt[0, 9]


@gpu
def test_sample_ctl_automaton_launcher_refuses_bad_arguments(ext):
    z = torch.zeros(4096, dtype=torch.int32, device=DEV)
    base = dict(logits=z.data_ptr(), rf=z.data_ptr(), ids=z.data_ptr(), out=z.data_ptr(), alive=z.data_ptr(), N=1, V=256,
                step=0, max_len=4, eos=0, inv_temp=z.data_ptr(), top_k=z.data_ptr(), top_p=z.data_ptr(), plen=z.data_ptr(),
                prefix=z.data_ptr())
    full = dict(allow_tab=z.data_ptr(), allow_state=z.data_ptr(), allow_next=z.data_ptr(), allow_rows=1)
    for bad in (dict(full, allow_next=0), dict(full, allow_state=0), dict(full, allow_tab=0),
                dict(full, allow_idx=z.data_ptr()), dict(full, allow_rows=0), dict(full, allow_rows=65536)):
        with pytest.raises(RuntimeError):
            ext.sample_ctl(dict(base, **bad), stream())
    with pytest.raises(RuntimeError):                                    # V = 64 has no automaton instantiation
        ext.sample_ctl(dict(base, V=64, **full), stream())


# ------------------------------------------------------------------------------- beam kernels
def auto_step(c, seed):
    """br.step_inputs plus a state per beam row: sets as cg.masked_step's per name, but beam 1 of every name
    (where W > 1) sits in a state whose line is empty -- a live beam whose every child is masked -- and beam 0
    of name 2 in the free state.  The forced char of a name lies in its beams' sets (but the empty one)."""
    d = br.step_inputs(c, seed)
    rng = np.random.default_rng(seed + 31 * c.V + c.W)
    N, W, V = c.N, c.W, c.V
    A = np.zeros((N, W, V), bool)
    for n in range(N):
        for b in range(W):
            if n % 3 == 0:
                A[n, b, rng.choice(np.arange(1, V), 2, replace=False)] = True
            elif n % 3 == 1:
                A[n, b, 1:] = rng.random(V - 1) < 0.5
            else:
                A[n, b] = True
            if d["step"] < d["plen"][n]:
                A[n, b, int(d["prefix"][n, d["step"]])] = True
        if W > 1:
            A[n, 1] = False
    d["allowed"] = A
    S = 300
    lines = rng.random((S, V)) < 0.5
    lines[0] = True
    where = rng.choice(np.arange(1, S - 1), N * W, replace=False)
    where[N * W - 1] = S - 1
    flat = A.reshape(N * W, V)
    for i, w in enumerate(where):
        if flat[i].all():
            where[i] = 0
    lines[where[where > 0]] = flat[where > 0]
    d["tab"], d["nxt"], d["astate"] = pack(lines), rng.integers(0, S, (S, V)).astype(np.uint16), where.astype(np.int32)
    return d


def run_select_auto(ext, d, astate=None, rows=None):
    R, V, W, N = d["R"], d["V"], d["W"], d["N"]
    lg, scr, st = t(d["logits"]), t(d["score"]), t(d["state"])
    pl, pre = t(d["plen"]), t(d["prefix"])
    out_f = torch.full((R + 3,), float("nan"), device=DEV)
    outs = {k: torch.full((R + 3,), -77, dtype=torch.int32, device=DEV)
            for k in ("parent", "chr", "state_out", "next_id", "sel", "allow_state_out")}
    lp = torch.full((R + 3, V), float("nan"), device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    dt, dn = t(d["tab"].view(np.int32)), t(d["nxt"].view(np.int16))
    sin = t(d["astate"] if astate is None else astate)
    a = dict(logits=lg.data_ptr(), splits=d["splits"], slab=d["Rp"] * V, score_in=scr.data_ptr(), state_in=st.data_ptr(),
             plen=pl.data_ptr(), prefix=pre.data_ptr(), score_out=out_f.data_ptr(), err=err.data_ptr(), lp=lp.data_ptr(),
             N=N, W=W, V=V, step=d["step"], max_len=d["ML"], sos=d["sos"], eos=d["eos"], allow_tab=dt.data_ptr(),
             allow_next=dn.data_ptr(), allow_state_in=sin.data_ptr(), allow_rows=d["tab"].shape[0] if rows is None else rows,
             **{k: v.data_ptr() for k, v in outs.items()})
    if d["bias"] is not None:
        b = t(d["bias"])
        a["bias"] = b.data_ptr()
    ext.beam_select(a, stream())
    torch.cuda.synchronize()
    return dict(score=out_f.cpu().numpy(), parent=outs["parent"].cpu().numpy(), chr=outs["chr"].cpu().numpy(),
                state=outs["state_out"].cpu().numpy(), next_id=outs["next_id"].cpu().numpy(), sel=outs["sel"].cpu().numpy(),
                lp=lp.cpu().numpy(), err=err.cpu().numpy(), astate=outs["allow_state_out"].cpu().numpy(),
                astate_in=sin.cpu().numpy())


def child_states(d, ref, astate=None):
    """The rule: nxt[parent's state][chr] for an extension, 0 for a carry or a dead slot."""
    W = d["W"]
    src = d["astate"] if astate is None else astate
    out = np.zeros(d["R"], np.int32)
    for i in range(d["R"]):
        if ref["parent"][i] >= 0 and ref["chr"][i] >= 0:
            out[i] = d["nxt"][src[i // W * W + ref["parent"][i]], ref["chr"][i]]
    return out


AUTO_CASES = [br.StepCase(256, W, 3, 1 + i % 2, i % 3 == 1, mode, states, (5, 0)[i % 2])
              for i, (W, mode, states) in enumerate([(1, "free", "live"), (4, "free", "mix"), (4, "mixed", "live"),
                                                     (32, "free", "mix"), (32, "forced", "mix"), (17, "free", "step0")])]
AUTO_CASES.append(br.StepCase(512, 4, 3, 1, False, "free", "mix", 5))


@pytest.mark.parametrize("i", range(len(AUTO_CASES)), ids=lambda i: "-".join(map(str, AUTO_CASES[i])))
def test_auto_select_inputs_clear_the_guard(i):
    d = br.plant_step(auto_step(AUTO_CASES[i], i % 3))
    ref = br.select_ref(d)
    assert (ref["clear"] >= br.GUARD).all()
    W, V = d["W"], d["V"]
    for k in range(d["R"]):
        if ref["chr"][k] >= 0:
            assert d["allowed"][k // W, ref["parent"][k], ref["chr"][k]]     # inside the parent's own set
            assert W == 1 or ref["parent"][k] != 1                           # the all-masked beam has no child
    # the planted lines are the rows' sets
    lines = cpu_ref.Automaton(d["tab"], d["nxt"], np.zeros(1, np.int32)).lines()
    assert np.array_equal(lines[d["astate"]], d["allowed"].reshape(d["R"], V))


@gpu
@pytest.mark.parametrize("i", range(len(AUTO_CASES)), ids=lambda i: "-".join(map(str, AUTO_CASES[i])))
def test_auto_select_matches_fp64_rule_and_writes_the_childrens_states(ext, i):
    d = br.plant_step(auto_step(AUTO_CASES[i], i % 3))
    ref = br.select_ref(d)
    got = run_select_auto(ext, d)
    R = d["R"]
    own = {k: (v[:R] if k != "err" else v) for k, v in got.items()}
    assert br.check_step(ref, own) == []
    assert (got["err"] == 0).all()
    assert np.array_equal(own["astate"], child_states(d, ref))
    assert (got["astate"][R:] == -77).all() and np.array_equal(got["astate_in"], d["astate"])   # never in place
    assert np.isnan(got["score"][R:]).all() and all((got[k][R:] == -77).all() for k in ("parent", "chr", "state", "next_id", "sel"))


@gpu
def test_auto_select_flags_a_state_outside_the_table_and_reset_plants_the_starts(ext):
    c = br.StepCase(256, 3, 3, 1, False, "free", "live", 5)
    d = auto_step(c, 1)
    for bad in (d["tab"].shape[0], -3):
        st = d["astate"].copy()
        st[4] = bad                                                      # name 1, beam 1
        got = run_select_auto(ext, d, st)
        assert got["err"][0] == 16 and got["err"][1] == np.int32(bad) and got["err"][2] == 4
        free = d["allowed"].copy()
        free[1, 1] = True                                                # the beam takes line 0
        ref = br.select_ref(dict(d, allowed=free))
        assert br.check_step(ref, {k: got[k][:d["R"]] for k in ("score", "parent", "chr", "state", "next_id", "sel", "lp")}) == []
        st0 = st.copy()
        st0[4] = 0
        assert np.array_equal(got["astate"][:d["R"]], child_states(d, ref, st0))
    z = torch.zeros(256, dtype=torch.int32, device=DEV)
    base = dict(logits=z.data_ptr(), score_in=z.data_ptr(), state_in=z.data_ptr(), plen=z.data_ptr(), prefix=z.data_ptr(),
                score_out=z.data_ptr() + 64, parent=z.data_ptr(), chr=z.data_ptr(), state_out=z.data_ptr() + 64,
                next_id=z.data_ptr(), N=1, W=2, V=256, step=0, max_len=4, sos=1, eos=0)
    full = dict(allow_tab=z.data_ptr(), allow_next=z.data_ptr(), allow_state_in=z.data_ptr(), allow_state_out=z.data_ptr() + 128,
                allow_rows=1)
    for bad in (dict(full, allow_next=0), dict(full, allow_state_out=0), dict(full, allow_state_out=z.data_ptr()),
                dict(full, allow_idx=z.data_ptr()), dict(full, allow_tab=0)):
        with pytest.raises(RuntimeError):
            ext.beam_select(dict(base, **bad), stream())
    # beam_reset: beam 0 of name n in start[n], every other row -- padding included -- in state 0
    N, W, Bp, H = 5, 3, 64, 64
    h = torch.ones(Bp, H, device=DEV)
    ints = {k: torch.full((Bp + 1,), -5, dtype=torch.int32, device=DEV) for k in ("ids", "state", "len", "allow_state")}
    score = torch.ones(Bp, device=DEV)
    rows = torch.ones(Bp, 7, dtype=torch.uint8, device=DEV)
    start = t(np.array([7, 0, 2999, 1, 65534], np.int32))
    ext.beam_reset(dict(N=N, W=W, L=1, Bp=Bp, H=H, max_len=6, sos=1, h=[h.data_ptr()], score=score.data_ptr(),
                        rows=rows.data_ptr(), allow_start=start.data_ptr(), **{k: v.data_ptr() for k, v in ints.items()}), stream())
    torch.cuda.synchronize()
    want = np.zeros(Bp, np.int32)
    want[0:N * W:W] = [7, 0, 2999, 1, 65534]
    a = ints["allow_state"].cpu().numpy()
    assert np.array_equal(a[:Bp], want) and a[Bp] == -5 and ints["state"].cpu().numpy()[:N * W:W].tolist() == [1] * N
    with pytest.raises(RuntimeError):
        ext.beam_reset(dict(N=N, W=W, L=1, Bp=Bp, H=H, max_len=6, sos=1, h=[h.data_ptr()], score=score.data_ptr(),
                            rows=rows.data_ptr(), **{k: v.data_ptr() for k, v in ints.items()}), stream())


# ------------------------------------------------------------------------------- HipGenerator.generate
CFG = sc.CFG          # GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10)
BAR = sc.BAR
ABC3 = ["".join(w) for L in range(4) for w in __import__("itertools").product("abc", repeat=L)]      # 40 names
EXCLUDED = ABC3[::2]
RXS = [".*son", ".*ann.*", "Ma[rl][a-z]{2,4}", None, None]
SETS = [LETTERS, LOWER, None, None, "abc"]
EXS = [None, None, ["Maria", "Marab"], None, EXCLUDED]
MAXS = [None, 8, None, None, 3]
PRES = ["", "ab", "Ma", "Qu", "c"]


def mixture(N, shift=0):
    """make_constraints keywords, prefixes and per-name controls of N names; name n is of kind (n + n // 64 +
    shift) % 5 -- a suffix, a contains, a counted regex with two exclusions, a free name, a small exclusion
    language -- so a batch that read rows 0.. would follow another name's language.  Every third name has
    its kind's prefix."""
    kind = [(n + n // 64 + shift) % 5 for n in range(N)]
    cons = dict(regex=[RXS[k] for k in kind], charset=[SETS[k] for k in kind], exclude=[EXS[k] for k in kind],
                max_len=[MAXS[k] for k in kind])
    ctl = dict(prefix=[PRES[k] if n % 3 == 0 else "" for n, k in enumerate(kind)],
               temperature=[(0.8, 1.0, 0.0, 1.3)[n % 4] for n in range(N)], top_k=[(0, 20, 5)[n % 3] for n in range(N)],
               top_p=[(1.0, 0.9)[n % 2] for n in range(N)])
    return kind, cons, ctl


def names_of(rows):
    return [bytes(r[:CFG.max_len]).split(b"\0")[0].decode("latin-1") for r in rows]


def all_in_language(rows, kind, ctl=None):
    """No tolerance: Python's re on the whole name, the exclusion list, the length bounds, the prefix."""
    for n, nm in enumerate(names_of(rows)):
        k = kind[n]
        if RXS[k] is not None and not re.fullmatch(RXS[k], nm):
            return f"name {n} {nm!r} does not match {RXS[k]!r}"
        if SETS[k] is not None and RXS[k] is None and not all(ch in SETS[k] for ch in nm):
            return f"name {n} {nm!r} leaves its charset"
        if nm in (EXS[k] or []):
            return f"name {n} {nm!r} is excluded"
        if len(nm) > (MAXS[k] or CFG.max_len):
            return f"name {n} {nm!r} is too long"
        if ctl is not None and not nm.startswith(ctl["prefix"][n]):
            return f"name {n} {nm!r} lost its prefix"
    return None


def test_the_mixture_bites_in_the_fp64_oracle():
    """A condition of the GPU tests below, on the CPU: without the constraints the same uniforms leave the
    languages, the exclusion list included."""
    N = 1000
    rf = random_floats(N, CFG.max_len, seed=9)
    kind, cons, ctl = mixture(N)
    plain = sc.oracle(("aut1000", "plain"), False, rf, **ctl)
    assert all_in_language(plain, kind) is not None
    small = [n for n in range(N) if kind[n] == 4]
    free = sc.oracle(("aut1000", "abc"), False, rf, constraints=dict(charset=[SETS[k] for k in kind], max_len=[MAXS[k] for k in kind]), **ctl)
    assert any(names_of(free[small])[i] in EXCLUDED for i in range(len(small)))
    want = sc.oracle(("aut1000", 0), False, rf, constraints=cons, **ctl)
    assert all_in_language(want, kind, ctl) is None
    assert len({nm for nm in names_of(want[small])}) > 5


@gpu
def test_generate_1000_names_of_the_mixture_match_fp64_oracle_and_stay_in_their_languages():
    N = 1000
    rf = random_floats(N, CFG.max_len, seed=9)
    kind, cons, ctl = mixture(N)
    gen = sc.make_gen(max_batch=256)                                     # batches of 256, 256, 256, 232
    got = gen.generate(rf, constraints=cons, **ctl)
    assert gen.g.read_error() == 0
    assert all_in_language(got, kind, ctl) is None                       # 100 %, no tolerance
    assert gen.g.automaton_graphs() == 2 and gen.g.ctl_graphs() == 0
    s = sc.same(got, sc.oracle(("aut1000", 0), False, rf, constraints=cons, **ctl))
    print("automaton-constrained names identical to the fp64 oracle:", s)
    assert s >= BAR
    # the Automaton object in place of the keywords, and a replay: the same bytes
    aut = cpu_ref.make_constraints(CFG, N, **cons)
    assert (gen.generate(rf, constraints=aut, **ctl) == got).all() and gen.g.automaton_graphs() == 2
    wrong = mixture(N, shift=1)[0]
    assert all_in_language(got, wrong) is not None


@gpu
def test_generate_40_names_take_the_per_char_graph_and_leave_the_other_paths_alone():
    N = 40
    rf = random_floats(N, CFG.max_len, seed=9)
    kind, cons, ctl = mixture(N)
    gen = sc.make_gen()
    assert gen.g.uses_persist_ctl(N)
    before = gen.generate(rf)
    before_ctl = gen.generate(rf, temperature=0.7, prefix="Jo")
    assert gen.g.ctl_workspace_bytes() == 0 and gen.g.ctl_graphs() == 0 and gen.g.automaton_graphs() == 0
    got = gen.generate(rf, constraints=cons, **ctl)
    assert gen.g.read_error() == 0 and all_in_language(got, kind, ctl) is None
    assert gen.g.automaton_graphs() == 1 and gen.g.ctl_graphs() == 0 and gen.g.ctl_workspace_bytes() > 0
    want = sc.oracle(("aut40", 0), False, rf, constraints=cons, **ctl)
    print("40 automaton-constrained names identical to the fp64 oracle:", sc.same(got, want))
    # the unconstrained paths after it: the persistent launches, the bytes they gave before
    assert gen.g.uses_persist_ctl(N) and gen.g.uses_persist(N)
    assert (gen.generate(rf) == before).all()
    assert (gen.generate(rf, temperature=0.7, prefix="Jo") == before_ctl).all()
    assert gen.g.ctl_graphs() == 0 and gen.g.automaton_graphs() == 1 and gen.g.read_error() == 0
    # a per-position constraint next to it keeps its own graph
    pos = gen.generate(rf, constraints=dict(pattern="[A-Z]", charset=LOWER, min_len=4, max_len=7))
    assert gen.g.ctl_graphs() == 1 and gen.g.automaton_graphs() == 1
    assert all(re.fullmatch("[A-Z][a-z]{3,6}", nm) for nm in names_of(pos))


AS_REGEX = dict(regex="[A-Z][a-z]{3,6}")
AS_PATTERN = dict(pattern="[A-Z]", charset=LOWER, min_len=4, max_len=7)


@gpu
@pytest.mark.parametrize("N", [40, 300])
def test_regex_and_pattern_spellings_are_bitwise_identical_on_the_device(N):
    """The masks are equal at every step, so the arithmetic is the same: tolerance 0."""
    rf = random_floats(N, CFG.max_len, seed=11)
    gen = sc.make_gen(max_batch=128)
    for ctl in ({}, dict(temperature=0.8, top_k=40, top_p=0.95), dict(temperature=0.0, prefix="Ma")):
        a = gen.generate(rf, constraints=AS_REGEX, **ctl)
        b = gen.generate(rf, constraints=AS_PATTERN, **ctl)
        assert np.array_equal(a, b)
        assert all(re.fullmatch("[A-Z][a-z]{3,6}", nm) for nm in names_of(a))
    assert gen.g.read_error() == 0
    if N == 40:
        g = gen_beam()
        for pre, W in (([""], 8), (["", "M", "Jo", "Anna"], 4)):
            a = g.beam_search(pre, width=W, constraints=AS_REGEX)
            b = g.beam_search(pre, width=W, constraints=AS_PATTERN)
            assert np.array_equal(a.rows, b.rows) and np.array_equal(a.logp.view(np.uint32), b.logp.view(np.uint32))
            assert np.array_equal(a.n_tok, b.n_tok) and np.array_equal(a.n_beams, b.n_beams)
        assert g.g.read_error() == 0


@gpu
def test_exclude_emitted_over_three_batches_yields_no_duplicate(tmp_path):
    """`generate --exclude-emitted` on the device: a language of 39 names, 30 of them in three batches."""
    from gru_mpi_cuda_amd import cli
    from gru_mpi_cuda_amd.utils import ckpt
    m = str(tmp_path / "model.bin")
    ckpt.save(m, CFG, sc.model())
    out = str(tmp_path / "names.txt")
    assert cli.main(["generate", "--ckpt", m, "-n", "30", "--seed", "3", "--charset", "abc", "--max-name-len", "3",
                     "--min-len", "1", "--exclude-emitted", "--emit-batch", "10", "--out", out]) == 0
    names = open(out).read().splitlines()
    assert len(names) == 30 and len(set(names)) == 30 and all(re.fullmatch("[abc]{1,3}", nm) for nm in names), names


# ------------------------------------------------------------------------------- HipGenerator.beam_search
BEAM_MODEL = cg.BEAM_MODEL
BEAM_CASES = {
    "son-W4": (["", "J"], 4, dict(regex=".*son", charset=LETTERS)),
    "mixed-W6": (["", "Ma", "", "c", "q"], 6,
                 dict(regex=[".*ann.*", "Ma[rl][a-z]{2,4}", None, None, "[a-z]{2,3}"], charset=[LOWER, None, None, "abc", None],
                      exclude=[None, ["Maria"], None, EXCLUDED, ["qa", "qb"]], max_len=[8, None, None, 3, None])),
    "fewer-than-W": (["", "Ma"], 8, dict(regex="M[ae][xy]", exclude=["Mex"])),
}
_orc = {}


def gen_beam():
    from test_beam_gpu import gen_of
    return gen_of(BEAM_MODEL)


def beam_oracle(name):
    if name not in _orc:
        cfg, p = br.case_model(BEAM_MODEL)
        pre, W, kw = BEAM_CASES[name]
        _orc[name] = br.oracle(p, cfg, pre, W, constraints=kw)
    return _orc[name]


def beam_language_errors(name, got):
    pre, W, kw = BEAM_CASES[name]
    bad = []
    for n, row in enumerate(got.names()):
        rx = kw["regex"][n] if isinstance(kw["regex"], list) else kw["regex"]
        ex = kw["exclude"][n] if "exclude" in kw and isinstance(kw["exclude"][0], (list, type(None))) else kw.get("exclude")
        for nm in row:
            if rx is not None and not re.fullmatch(rx, nm):
                bad.append((n, nm, rx))
            if nm in (ex or []):
                bad.append((n, nm, "excluded"))
    return bad


@pytest.mark.parametrize("name", list(BEAM_CASES))
def test_beam_cases_are_settled_in_the_fp64_oracle(name):
    orc = beam_oracle(name)
    assert int((~orc["settled"]).sum()) * 8 <= len(BEAM_CASES[name][0]), orc["clear"].min(1)
    cfg, p = br.case_model(BEAM_MODEL)
    res = cpu_ref.BeamResult(orc["rows"], orc["logp"], orc["n_tok"], orc["n_beams"], cfg.eos)
    assert beam_language_errors(name, res) == []
    # the extended reference model and cpu_ref.beam_search are one rule
    pre, W, kw = BEAM_CASES[name]
    twin = cpu_ref.beam_search({k: v.double() for k, v in p.items()}, cfg, pre, W, constraints=kw)
    assert np.array_equal(twin.rows, orc["rows"]) and np.array_equal(twin.n_beams, orc["n_beams"])


@gpu
@pytest.mark.parametrize("name", list(BEAM_CASES))
def test_beam_search_with_an_automaton_matches_fp64_oracle(name):
    cfg, p = br.case_model(BEAM_MODEL)
    pre, W, kw = BEAM_CASES[name]
    g = gen_beam()
    got = g.beam_search(pre, width=W, constraints=kw)
    assert g.g.read_error() == 0
    orc = beam_oracle(name)
    assert br.check_result(cfg, pre, orc, got, br.score64_of(p, cfg, got)) == []
    assert beam_language_errors(name, got) == []
    if name == "fewer-than-W":
        assert got.n_beams.tolist() == [3, 2]
        assert sorted(got.names()[0]) == ["Max", "May", "Mey"] and sorted(got.names()[1]) == ["Max", "May"]
        assert np.isneginf(got.logp[0, 3:]).all() and (got.rows[0, 3:] == 0).all()
    aut = cpu_ref.make_constraints(cfg, len(pre), **kw)
    again = g.beam_search(pre, width=W, constraints=aut)                 # the object form, a replay
    assert np.array_equal(again.rows, got.rows) and np.array_equal(again.logp.view(np.uint32), got.logp.view(np.uint32))
    plain = g.beam_search(pre, width=W)
    assert g.g.read_error() == 0 and br.check_result(cfg, pre, br.oracle(p, cfg, pre, W), plain) == []


# ------------------------------------------------------------------------------- HipGenerator.score
@gpu
def test_score_with_a_regex_matches_fp64_oracle_and_rows_outside_are_minus_infinity():
    """300 rows the fp64 sampler drew from the language, in batches of 64, under tests/test_score_ctl_gpu.py's
    check and tolerance; then rows outside the language."""
    import test_score_ctl_gpu as tg
    from gru_mpi_cuda_amd.engine.generator import encode_names
    N = 300
    kw = dict(temperature=0.8, top_k=40, top_p=0.95)
    cons = dict(regex=".*an.*|[A-Z][a-z]{3,6}", charset=LETTERS, exclude=["Anna", "an"])
    rows = tsc.oracle_rows("aut-score", N, 9, constraints=cons, **kw)
    gen = sc.make_gen(sharp=True, max_batch=64)
    res = gen.score(rows, constraints=cons, **kw)
    assert gen.g.read_error() == 0
    walked = cpu_ref.make_constraints(CFG, N, **cons).for_rows(CFG, rows)   # the oracle's and the guard's view of it
    tg.check_settled(res, "aut-score", rows, dict(kw, constraints=walked), kw["temperature"], "regex score")
    out = encode_names(["Anna", "an", "Hann", "x", "Bo", "Bob9", "Bobby"], CFG)
    r2 = gen.score(out, constraints=cons)                                # (no top-k / top-p: inside the language is finite)
    want = cpu_ref.score(tsc.p64(), CFG, out, constraints=cons)
    assert np.isneginf(want[1][[0, 1, 3, 4, 5]]).all() and np.isfinite(want[1][[2, 6]]).all()
    assert np.array_equal(np.isneginf(r2.name_logp), np.isneginf(want[1])) and r2.impossible == 5
    assert np.array_equal(np.isneginf(r2.tok_logp), np.isneginf(want[0]))


@gpu
def test_a_growing_exclusion_list_keeps_a_bounded_number_of_recordings():
    """Every state count records a graph of its own; a caller whose list grows call by call never returns to
    one, so a full map (16) is dropped before the next recording.  The names stay right across the drop."""
    N = 40
    rf = random_floats(N, CFG.max_len, seed=5)
    gen = sc.make_gen()
    seen = set()
    for k in range(1, 21):                                               # 20 calls, 20 state counts
        ex = [c + c for c in LOWER[:k]]                                  # "aa", "bb", ...: a state per first letter
        rows = gen.generate(rf, constraints=dict(regex="[a-z]{2,3}", exclude=ex), temperature=0.9)
        names = names_of(rows)
        assert all(re.fullmatch("[a-z]{2,3}", nm) and nm not in ex for nm in names), (k, names)
        seen.add(cpu_ref.make_constraints(CFG, N, regex="[a-z]{2,3}", exclude=ex).states)
        assert 1 <= gen.g.automaton_graphs() <= 16
    assert len(seen) > 16 and gen.g.read_error() == 0                    # more state counts than the map holds

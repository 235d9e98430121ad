"""Sampling controls on the CPU reference path (docs/DESIGN.md §4b): cpu_ref.filter_probs /
sample_controlled against a brute-force sort-based implementation of the same set definitions,
controlled cpu_ref.generate (neutral controls, greedy, prefixes, uniforms by position), the CLI flags
and every validation error."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.engine import generator as G
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt
from gru_mpi_cuda_amd.utils.data import random_floats


def brute_keep(x, T, k, p):
    """The kept set by sorting: walk the values in descending order, group by group of equal values."""
    x = [float(v) for v in x]
    V = len(x)
    if T == 0:
        return {x.index(max(x))}
    inv = float(np.float32(1.0 / T))
    y = [v * inv for v in x]
    order = sorted(range(V), key=lambda i: -y[i])
    keep = set(range(V))
    if 0 < k < V:
        keep, j = set(), 0
        while j < V and len(keep) < k:        # whole groups of ties until k values are in
            g = [i for i in order if y[i] == y[order[j]]]
            keep |= set(g)
            j += len(g)
    m = max(y)
    e = {i: np.exp(y[i] - m) for i in keep}
    tot = sum(e.values())
    q = {i: e[i] / tot for i in keep}
    if p < 1:
        kept, mass = set(), 0.0
        for v in sorted(set(q.values()), reverse=True):   # groups of equal q, largest first
            if not mass < p:
                break
            g = [i for i in keep if q[i] == v]
            kept |= set(g)
            mass += v * len(g)
        keep = kept
    return keep


def brute_probs(x, T, k, p):
    keep = brute_keep(x, T, k, p)
    if T == 0:
        y = [float(v) for v in x]
    else:
        inv = float(np.float32(1.0 / T))
        y = [float(v) * inv for v in x]
    m = max(y)
    e = np.array([np.exp(y[i] - m) if i in keep else 0.0 for i in range(len(x))])
    return e / e.sum(), keep


ROWS = {
    "tie_at_k": [1.0, 3.0, 2.0, 2.0, 0.5, -1.0, 2.5, 0.0],         # k = 3: the two 2.0 straddle third place
    "distinct": [0.3, -0.2, 1.7, 0.9, 2.4, -1.1, 0.0, 1.2],
    "tie_at_p": [2.0, 1.0, 1.0, 0.0, -3.0, -3.0, -8.0, -8.0],      # the two 1.0 straddle the p = 0.7 edge
    "all_equal": [0.5] * 8,
    "negative_zero": [-0.0, 0.0, -1.0, 1.0, -2.0, 0.0, -0.0, 0.5],
}


@pytest.mark.parametrize("name", sorted(ROWS))
@pytest.mark.parametrize("T", [0.0, 0.5, 1.0, 2.0])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 7, 8, 15])
@pytest.mark.parametrize("p", [1e-6, 0.5, 0.7, 0.9, 1.0])
def test_filter_probs_matches_brute_force(name, T, k, p):
    x = ROWS[name]
    want, keep = brute_probs(x, T, k, p)
    got = cpu_ref.filter_probs(torch.tensor(x, dtype=torch.float64), T, k, p)
    assert set(np.nonzero(got.numpy())[0].tolist()) == keep
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=0)
    got32 = cpu_ref.filter_probs(torch.tensor(x, dtype=torch.float32), T, k, p)
    assert set(np.nonzero(got32.numpy())[0].tolist()) == keep      # ties: the same set in fp32 and fp64
    np.testing.assert_allclose(got32.numpy(), want, rtol=2e-6, atol=0)


def test_filter_probs_edges_by_hand():
    f = lambda x, *c: set(np.nonzero(cpu_ref.filter_probs(torch.tensor(x, dtype=torch.float64), *c).numpy())[0].tolist())
    x = ROWS["tie_at_k"]
    assert f(x, 1.0, 3, 1.0) == {1, 6, 2, 3}                 # the tie at third place keeps both
    assert f(x, 1.0, 2, 1.0) == {1, 6}
    assert f(x, 1.0, 1, 1.0) == {1}
    assert f(x, 1.0, 8, 1.0) == f(x, 1.0, 0, 1.0) == f(x, 1.0, 99, 1.0) == set(range(8))
    assert f(ROWS["all_equal"], 1.0, 1, 1.0) == set(range(8))   # all tied with the first: all kept
    y = ROWS["tie_at_p"]
    q = torch.softmax(torch.tensor(y, dtype=torch.float64), -1)
    assert q[0] < 0.7 < q[0] + q[1]                          # the edge falls inside the tied pair
    assert f(y, 1.0, 0, 0.7) == {0, 1, 2}                    # both kept
    assert f(y, 1.0, 0, 1e-6) == {0}                         # a tiny p keeps the maximum: never empty
    assert f(y, 1.0, 0, 1.0) == set(range(8))
    assert f(y, 0.0) == {0} and f(ROWS["all_equal"], 0.0) == {0}   # greedy: the lowest arg-max index
    # temperature, then top-k, then top-p: p applies to the softmax of the top-k set
    z = [2.0, 1.0, 0.0, -1.0]
    q2 = torch.softmax(torch.tensor(z[:2], dtype=torch.float64) * float(np.float32(2.0)), -1)
    assert q2[0] > 0.85 and f(z, 0.5, 2, 0.85) == {0} and f(z, 0.5, 2, 0.9) == {0, 1}


def test_sample_controlled_rule_and_fallback():
    x = torch.tensor([ROWS["distinct"]] * 5, dtype=torch.float64)
    probs = cpu_ref.filter_probs(x[0], 1.0, 3, 1.0)
    kept = np.nonzero(probs.numpy())[0]                       # the three largest: 1.7, 2.4, 1.2
    assert kept.tolist() == [2, 4, 7]
    cs = np.cumsum(probs.numpy())
    r = torch.tensor([0.0, float(cs[2]) * 0.5, float(cs[2]) + 1e-9, 1.0, 1.5], dtype=torch.float64)
    sel = cpu_ref.sample_controlled(x, r, 1.0, 3, 1.0)
    # first index whose running sum exceeds r; r >= 1: the highest KEPT index, not V - 1
    assert sel.tolist() == [2, 2, 4, 7, 7]
    assert cpu_ref.sample_controlled(x, r, 1.0, 2, 1.0).tolist()[3:] == [4, 4]
    assert cpu_ref.sample_controlled(x[:1], torch.tensor([1.0], dtype=torch.float64)).tolist() == [7]   # nothing filtered: V - 1
    assert cpu_ref.sample_controlled(x[:1], torch.tensor([1.0], dtype=torch.float64), 0.0).tolist() == [4]


CFG = GRUConfig(vocab=256, embed=32, hidden=64, layers=2, max_len=10, sos=0, eos=0, seed=4)


@pytest.fixture(scope="module")
def model():
    params = init_params(CFG)
    params["fc.weight"] = params["fc.weight"] * 8   # a distribution with some shape to cut
    return params


def test_neutral_controls_are_bitwise_plain(model):
    rf = random_floats(60, CFG.max_len, seed=9)
    plain = cpu_ref.generate(model, CFG, rf)
    assert (cpu_ref.generate(model, CFG, rf, temperature=1.0, top_k=0, top_p=1.0, prefix="") == plain).all()
    assert (cpu_ref.generate(model, CFG, rf, top_k=np.full(60, 256)) == plain).all()
    p64 = {k: v.double() for k, v in model.items()}
    assert (cpu_ref.generate(p64, CFG, rf, temperature=1.0) == cpu_ref.generate(p64, CFG, rf)).all()
    assert (cpu_ref.generate(model, CFG, rf, 10, 20, top_p=1.0) == plain[10:30]).all()


def _argmax_chain(params, cfg, n):
    out = np.zeros((n, cfg.max_len + 1), np.uint8)
    x = [cfg.sos]
    for l in range(cfg.max_len):
        logits = cpu_ref.forward(params, cfg, torch.tensor([x]))[0, -1]
        c = int((logits == logits.max()).nonzero()[0][0])
        out[:, l] = c
        if c == cfg.eos:
            break
        x.append(c)
    return out


def test_greedy_is_the_argmax_chain(model):
    rf = random_floats(4, CFG.max_len, seed=1)
    p64 = {k: v.double() for k, v in model.items()}
    got = cpu_ref.generate(p64, CFG, rf, temperature=0.0)
    assert (got == _argmax_chain(p64, CFG, 4)).all()
    assert (cpu_ref.generate(p64, CFG, rf, top_k=1) == got).all()     # no exact ties in these logits
    assert (cpu_ref.generate(p64, CFG, 1.0 - rf, temperature=0.0) == got).all()   # the uniforms are ignored


def test_prefixes_and_uniforms_by_position(model):
    N, ML = 12, CFG.max_len
    rf = random_floats(N, ML, seed=5)
    pres = ["", "M", "Mar", "Mari", "abcdefghij", b"\x01\x02"] * 2
    rows, plen = G.encode_prefixes(pres, CFG)
    assert rows.shape == (N, ML) and plen.tolist() == [0, 1, 3, 4, 10, 2] * 2
    got = cpu_ref.generate(model, CFG, rf, prefix=pres, top_k=20)
    for i in range(N):
        assert (got[i, :plen[i]] == rows[i, :plen[i]]).all()
    assert bytes(got[4]) == b"abcdefghij\0"                   # exactly max_len chars: exactly that row
    # rows in the encode_names format are accepted too
    assert (cpu_ref.generate(model, CFG, rf, prefix=G.encode_names(pres, CFG), top_k=20) == got).all()
    # forced steps ignore their uniforms; the later steps still use their own positions
    rf2 = rf.copy().reshape(N, ML)
    for i in range(N):
        rf2[i, :plen[i]] = 0.999
    assert (cpu_ref.generate(model, CFG, rf2.reshape(-1), prefix=pres, top_k=20) == got).all()
    rf3 = rf.copy().reshape(N, ML)
    rf3[:, 5:] = 1.0 - rf3[:, 5:]
    alt = cpu_ref.generate(model, CFG, rf3.reshape(-1), prefix=pres, top_k=20)
    assert (alt[:, :5] == got[:, :5]).all() and not (alt == got).all()
    # an unprompted name next to prompted ones is the plain name
    assert (got[0] == cpu_ref.generate(model, CFG, rf, top_k=20)[0]).all()


def test_per_name_controls_match_one_by_one(model):
    N = 6
    rf = random_floats(N, CFG.max_len, seed=3)
    T = np.array([0.0, 0.5, 1.0, 2.0, 0.7, 1.0])
    k = np.array([0, 3, 40, 0, 1, 256])
    p = np.array([1.0, 0.9, 0.5, 0.3, 1.0, 1.0])
    pre = ["", "A", "", "Bo", "", "C"]
    got = cpu_ref.generate(model, CFG, rf, temperature=T, top_k=k, top_p=p, prefix=pre)
    for i in range(N):
        one = cpu_ref.generate(model, CFG, rf, i, 1, temperature=T[i], top_k=int(k[i]), top_p=p[i], prefix=pre[i])
        assert (one[0] == got[i]).all()


def test_namegen_world1_and_cli(tmp_path, model):
    from gru_mpi_cuda_amd.parallel.dist import DistCtx
    m = str(tmp_path / "model.bin")
    ckpt.save(m, CFG, model, fmt="gen")
    N, ML = 7, CFG.max_len
    rf = random_floats(N, ML, seed=2)
    k = np.arange(1, N + 1)
    pre = ["Ma", "", "Jo", "", "", "Kat", ""]
    want = cpu_ref.generate(model, CFG, rf, temperature=0.8, top_k=k, top_p=0.95, prefix=pre)
    G.namegen_initialize(N, 0, m, ctx=DistCtx())
    out = np.zeros(N * (ML + 1), np.uint8)
    G.namegen(N, rf, out, temperature=0.8, top_k=k, top_p=0.95, prefix=pre)
    plain = np.zeros(N * (ML + 1), np.uint8)
    G.namegen(N, rf, plain)
    G.namegen_finalize()
    assert (out.reshape(N, ML + 1) == want).all()
    assert (plain.reshape(N, ML + 1) == cpu_ref.generate(model, CFG, rf)).all()
    # the CLI: flags for all names, and a prefix file cycled over the names
    raw = str(tmp_path / "raw.bin")
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", str(N), "--seed", "2", "--temperature", "0.8", "--top-k", "5",
                     "--top-p", "0.95", "--prefix", "Ma", "--raw-out", raw, "--out", str(tmp_path / "n.txt")]) == 0
    got = np.fromfile(raw, np.uint8).reshape(N, ML + 1)
    assert (got == cpu_ref.generate(model, CFG, rf, temperature=0.8, top_k=5, top_p=0.95, prefix="Ma")).all()
    assert all(ln.startswith("Ma") for ln in open(tmp_path / "n.txt").read().splitlines())
    pf = tmp_path / "pre.txt"
    pf.write_text("Ma\n\nJo\n")
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", str(N), "--seed", "2", "--top-k", "5",
                     "--prefix-file", str(pf), "--raw-out", raw, "--out", str(tmp_path / "n2.txt")]) == 0
    got = np.fromfile(raw, np.uint8).reshape(N, ML + 1)
    cyc = [["Ma", "", "Jo"][i % 3] for i in range(N)]
    assert (got == cpu_ref.generate(model, CFG, rf, top_k=5, prefix=cyc)).all()
    # without controls the CLI output is today's
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", str(N), "--seed", "2", "--raw-out", raw,
                     "--out", str(tmp_path / "n3.txt")]) == 0
    assert (np.fromfile(raw, np.uint8).reshape(N, ML + 1) == cpu_ref.generate(model, CFG, rf)).all()


@pytest.mark.parametrize("kw", [dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")),
                                dict(temperature=[1.0, -1.0, 1.0]), dict(top_k=-1), dict(top_k=[0, 2, -3]),
                                dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.2), dict(top_p=float("nan")),
                                dict(prefix="abcdefghijk"), dict(prefix=["a", "b\x00", "c"]),
                                dict(prefix=[b"a", b"\xff", b"c"]), dict(prefix=["a", "b"]),
                                dict(top_k=[1, 2])])
def test_bad_controls_raise(model, kw):
    cfg = CFG.replace(vocab=128) if "prefix" in kw and kw["prefix"][1:2] == [b"\xff"] else CFG
    rf = random_floats(3, cfg.max_len, seed=0)
    with pytest.raises(ValueError):
        cpu_ref.generate(model, cfg, rf, **kw)
    with pytest.raises(ValueError):
        cpu_ref.make_controls(cfg, 3, **kw)

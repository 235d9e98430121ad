"""Sampling controls on the persistent small-batch launch (gen_persist_ctl.hip, docs/DESIGN.md §4b).

Kernel level, as tests/test_gen_gpu.py: ``ext.gen_persist`` with the five control arrays on a
caller-owned, pre-filled workspace, canary-filled ``out`` / ``probs``, every state, logit, id, row and
probability checked by gen_ref.check_launch against the float64 CONTROLLED trajectory of
models/gen_ctl_ref.py (which plants the uniforms and keeps the kept sets clear of fp32 rounding;
tests/test_gen_ctl_ref.py shows the checker to fail on every planted defect).  A controlled launch
with neutral controls must leave every output byte and workspace word of the plain launch.

A prefix byte >= V (error value 16) cannot be expressed: the prefix is a byte array and the kernel
takes V = 256 or 512 only, so no test covers that branch.

Engine level: HipGenerator on the CFG of tests/test_sampling_ctl_gpu.py, batches of 64 names through
the controlled persistent launch against the fp64 cpu_ref.generate oracle, and the fallbacks.
"""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import gen_ctl_ref as cr
from gru_mpi_cuda_amd.models import gen_ref as gr
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32 = torch.int32
PROBS_CANARY = 0x7FC0A5A5      # a NaN bit pattern
OUT_CANARY = 0xA5
CTL_KEYS = ("inv_temp", "top_k", "top_p", "plen", "prefix")


def S():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def gp(ext):
    if ext.device_info()["cus"] < 256:
        pytest.skip("the persistent generator needs 256 compute units")
    return ext


def u32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _dev(d):
    up = lambda t: None if t is None else t.to(DEV).contiguous()
    return {k: ([up(t) for t in d[k]] if isinstance(d[k], list) else up(d[k])) for k in ("Whh", "Wih", "bhh", "bih", "Wfc", "bfc", "P")}


def _ptrs(ts):
    return [0 if t is None else t.data_ptr() for t in ts]


def _new_ws(ext, H, L, V, ML):
    ws = torch.zeros(ext.gen_persist_ws_floats(H, L, V, ML), dtype=I32, device=DEV)
    ext.gen_persist_fill_ws(ws.data_ptr(), H, L, V, ML, S())
    sync = torch.zeros(ext.gen_persist_sync_words(L), dtype=I32, device=DEV)
    torch.cuda.synchronize()
    return ws, sync


def _run(ext, d, rf, ctl, probs, ws=None, sync=None, par=0):
    """One launch on the inputs d (controlled when ctl is given) -> the buffers check_launch reads."""
    H, L, V, N, ML = d["H"], d["L"], d["V"], d["N"], d["ML"]
    w = _dev(d)
    if ws is None:
        ws, sync = _new_ws(ext, H, L, V, ML)
    Np = (N + 15) // 16 * 16
    err = torch.zeros(4, dtype=I32, device=DEV)
    out = torch.full((N + 2, ML + 1), OUT_CANARY, dtype=torch.uint8, device=DEV)
    rfd = torch.from_numpy(rf).to(DEV).contiguous()
    a = dict(N=N, H=H, L=L, V=V, ML=ML, sos=d["sos"], eos=d["eos"], par=par, Whh=_ptrs(w["Whh"]), bhh=_ptrs(w["bhh"]),
             Wih=_ptrs(w["Wih"]), bih=_ptrs(w["bih"]), Wfc=w["Wfc"].data_ptr(), bfc=w["bfc"].data_ptr(), P=w["P"].data_ptr(),
             rf=rfd.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), sync=sync.data_ptr(), err=err.data_ptr())
    held = []
    if ctl is not None:
        for k in CTL_KEYS:
            if ctl.get(k) is not None:                            # (a missing array stays a null pointer)
                held.append(torch.from_numpy(np.ascontiguousarray(ctl[k])).to(DEV))
                a[k] = held[-1].data_ptr()
    pb = None
    if probs:
        pb = torch.full((Np + 2, V), PROBS_CANARY, dtype=I32, device=DEV)
        a["probs"] = pb.data_ptr()
    before = u32(ws)
    ext.gen_persist(a, S())
    torch.cuda.synchronize()
    got = dict(err=u32(err), sync=u32(sync), out=out.cpu().numpy(), out_canary=OUT_CANARY, par=par, ws_before=before,
               ws_after=u32(ws))
    if probs:
        got["probs"] = u32(pb).view(np.float32)
        got["probs_before"] = np.full((Np + 2, V), PROBS_CANARY, np.uint32).view(np.float32)
    return got


@functools.lru_cache(maxsize=None)
def _planted(c):
    """The case's inputs, its (possibly moved) controls and the float64 trajectory: computed once."""
    d = cr.case_inputs(c)
    ctl, orc = cr.plant(d, cr.controls(c), cr.case_plan(c))
    return d, ctl, orc


def _launch(ext, c, ws=None, sync=None, par=0):
    assert ext.gen_persist_ctl_supported(c.H, c.L, c.V, c.N, c.ML), c.name
    d, ctl, orc = _planted(c)
    got = _run(ext, d, orc["rf"], ctl, c.probs, ws, sync, par)
    fails, fig = gr.check_launch(d, orc, got, probs=c.probs, atol=cr.ATOL)
    T = gr.chars_run(orc["alive_after"], c.ML, c.probs)
    print(f"GENCTL {c.name:26s} par {par} chars {T}/{c.ML} moved {ctl['moved']} " +
          " ".join(f"{k} {v:9.3e} (atol {cr.ATOL[k]:.2e})" for k, v in fig.items()))
    assert not fails, f"{c.name}: " + "; ".join(fails)
    return got


# ====================================================================================== kernel level
@pytest.mark.parametrize("c", cr.CASES_A, ids=lambda c: c.name)
def test_ctl_every_variant(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", cr.CASES_B + cr.CASES_C, ids=lambda c: c.name)
def test_ctl_every_name_count_regime(gp, c):
    """H = 512: one name, direct, LDS-staged, distributed with two and three name tiles; H = 1024: the
    tagged state layout up to 8 names."""
    _launch(gp, c)


@pytest.mark.parametrize("H,L", gr.VARIANTS)
def test_ctl_vocab_512(gp, H, L):
    """Every variant the support function admits at V = 512, 5 and 33 names; the two it does not (their
    8-per-lane sampler spills: docs/DESIGN.md §4b) are refused by the launcher, not run."""
    cases = [c for c in cr.CASES_E if (c.H, c.L) == (H, L)]
    assert gp.gen_persist_supported(H, L, 512, 5, 4)
    assert gp.gen_persist_ctl_supported(H, L, 512, 5, 4) == bool(cases)
    if cases:
        assert [c.N for c in cases] == [5, 33]
        for c in cases:
            _launch(gp, c)
    else:
        c = cr.CtlCase("refused", H, L, 512, 5, 4)
        d = cr.case_inputs(c)
        with pytest.raises(RuntimeError):
            _run(gp, d, d["rf0"], cr.controls(c), True)


@pytest.mark.parametrize("c", cr.CASES_G, ids=lambda c: c.name)
def test_ctl_names_that_end(gp, c):
    """full-prefix: a name forced for all ML chars.  ends: every name has ended after char 1, half of them
    by an EOS byte inside a prefix of full length; with probs == nullptr the launch stops there although
    those names are still inside their prefix, with probs set it runs every char."""
    _launch(gp, c)


@pytest.mark.parametrize("c", cr.CASES_T, ids=lambda c: c.name)
def test_ctl_ties_at_the_maximum(gp, c):
    """Two FC rows are one row: greedy takes the lower index, top_k = 1 keeps both."""
    _launch(gp, c)


@pytest.mark.parametrize("c", cr.CASES_N, ids=lambda c: c.name)
def test_ctl_neutral_controls_are_the_plain_launch_bitwise(gp, c):
    d, ctl, orc = _planted(c)
    assert not ctl["moved"]
    plain = _run(gp, d, orc["rf"], None, True)
    got = _run(gp, d, orc["rf"], ctl, True)
    assert not gr.check_launch(d, orc, got)[0]                    # (gen_ref's own tolerances: a plain softmax row)
    for k in ("out", "err", "sync", "ws_before", "ws_after"):
        assert np.array_equal(plain[k], got[k]), k
    assert np.array_equal(plain["probs"].view(np.uint32), got["probs"].view(np.uint32))


def test_ctl_and_plain_launches_alternate_on_one_workspace(gp):
    """Parity 0, 1, 0, 1 on one workspace: plain (16 names), controlled (9, the tagged layout is N <= 8:
    plain rows here), controlled (8 names: tagged), plain (5 names), each fully checked."""
    H, L, V, ML = 1024, 2, 256, 4
    ws, sync = _new_ws(gp, H, L, V, ML)
    p0 = gr.Case("alt-plain-N16", H, L, V, 16, ML, 7, 3, seed_off=10)
    p1 = gr.Case("alt-plain-N5", H, L, V, 5, ML, seed_off=20)
    cases = {c.name: c for c in cr.CASES_C}

    def plain(c, par):
        d = gr.case_inputs(c)
        orc = gr.plant_uniforms(d)
        fails, _ = gr.check_launch(d, orc, _run(gp, d, orc["rf"], None, True, ws, sync, par))
        assert not fails, f"{c.name}: " + "; ".join(fails)

    plain(p0, 0)
    _launch(gp, cases["cc-N9"], ws, sync, 1)
    _launch(gp, cases["cc-N8"], ws, sync, 0)
    plain(p1, 1)


def test_ctl_binding_rejects_a_mixture_of_set_and_null_arrays(gp):
    c = cr.CASES_B[1]
    d, ctl, orc = _planted(c)
    for drop in CTL_KEYS:
        with pytest.raises(RuntimeError):
            _run(gp, d, orc["rf"], {k: v for k, v in ctl.items() if k != drop}, True)


# ====================================================================================== engine level
CFG = GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10, sos=0, eos=0, seed=4)
PREFIXES = ["Mar", "", "J", "Ka", "Eliz", "", "Bo", "abcdefghij"]
BAR = 0.995   # the project's fp32-vs-fp64 bar


@functools.lru_cache(maxsize=1)
def model():
    return init_params(CFG)


def make_gen(**kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    return HipGenerator(CFG, model(), precision="fp32", **kw)


@pytest.fixture
def pgen(gp):
    return make_gen(max_batch=64)


def test_generator_routes_small_controlled_batches_to_the_persistent_launch(pgen):
    g = pgen.g
    assert g.uses_persist_ctl(16) and g.uses_persist_ctl(64) and not g.uses_persist_ctl(65)
    g.set_persist_ctl_max(8)
    assert g.uses_persist_ctl(8) and not g.uses_persist_ctl(9) and g.uses_persist(9)
    g.set_persist_ctl_max(64)
    g.set_persist(False)
    assert not g.uses_persist_ctl(16) and not g.uses_persist(16)


def test_generator_prompted_names_through_persistent_batches_match_fp64_oracle(pgen):
    """1000 names through max_batch = 64: 16 controlled persistent launches (15 of 64 names, one of 40)
    on the caller's arrays at each batch's rows.  top_k = 20, top_p = 0.9, T = 0.8 at uniform seed 9 (fp32
    against fp64 on the CPU: 1000 of 1000, tests/test_sampling_ctl_gpu.py), with the prefixes on top."""
    N = 1000
    rf = random_floats(N, CFG.max_len, seed=9)
    pre = [PREFIXES[n % len(PREFIXES)] for n in range(N)]
    ctl = dict(top_k=20, top_p=0.9, temperature=0.8, prefix=pre)
    assert pgen.g.uses_persist_ctl(64) and pgen.g.uses_persist_ctl(N % 64)
    got = pgen.generate(rf, **ctl)
    assert pgen.g.read_error() == 0
    assert pgen.g.uses_persist_ctl(64)                            # no launch fell back
    assert pgen.g.ctl_workspace_bytes() == 0                      # the per-char path's staging was never allocated
    enc, plen = cpu_ref.encode_prefixes(pre, CFG)
    assert all((got[i, :plen[i]] == enc[i, :plen[i]]).all() for i in range(N))
    want = cpu_ref.generate({k: v.double() for k, v in model().items()}, CFG, rf, **ctl)
    s = float((got == want).all(1).mean())
    print("prompted top-k / top-p / temperature names identical to the fp64 oracle:", s)
    assert s >= BAR


def test_generator_spin_limit_falls_back_to_the_controlled_graph(gp):
    N = 48
    rf = random_floats(N, CFG.max_len, seed=13)
    ctl = dict(top_k=20, top_p=0.9, temperature=0.8, prefix=[PREFIXES[n % len(PREFIXES)] for n in range(N)])
    ref_gen = make_gen(max_batch=64)
    ref_gen.g.set_persist(False)
    want = ref_gen.generate(rf, **ctl)
    gen = make_gen(max_batch=64)
    assert gen.g.uses_persist_ctl(N)
    gen.g.inject_persist_error()
    got = gen.generate(rf, **ctl)
    assert (got == want).all()
    assert gen.g.read_error() == 0 and not gen.g.uses_persist_ctl(N) and not gen.g.uses_persist(N)
    assert gen.g.ctl_workspace_bytes() > 0


def test_generator_plain_and_controlled_calls_alternate(pgen):
    rf = random_floats(40, CFG.max_len, seed=9)
    before = pgen.generate(rf)
    a = pgen.generate(rf, temperature=0.7, prefix="Jo")
    b = pgen.generate(rf, temperature=0.7, prefix="Jo")
    assert (a == b).all() and (a[:, :2] == np.frombuffer(b"Jo", np.uint8)).all()
    assert (pgen.generate(rf) == before).all()
    neutral = pgen.generate(rf, temperature=1.0, top_k=0, top_p=1.0, prefix="")
    assert (neutral == before).all()                              # neutral controls: the plain launch's bytes
    assert pgen.g.read_error() == 0 and pgen.g.ctl_workspace_bytes() == 0

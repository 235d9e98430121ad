"""Soft controls inside the persistent small-batch launch (gen_persist_soft.hip, docs/DESIGN.md §4h), kernel
level.

As tests/test_gen_persist_con_gpu.py: ``ext.gen_persist`` with the five control arrays, the five soft keys
and -- in the constrained modes -- the constraint fields on a caller-owned, pre-filled workspace,
canary-filled ``out`` / ``probs`` / ``allow_state``, every state, logit, id, row and probability checked by
gen_ref.check_launch against the float64 ADJUSTED trajectory of models/gen_soft_ref.py (which plants the
uniforms on the adjusted distribution and keeps the kept sets clear of fp32 rounding;
tests/test_gen_soft_ref.py shows the checker to fail on every planted defect).
"""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import gen_con_ref as nr
from gru_mpi_cuda_amd.models import gen_ctl_ref as cr
from gru_mpi_cuda_amd.models import gen_ref as gr
from gru_mpi_cuda_amd.models import gen_soft_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32 = torch.int32
PROBS_CANARY = 0x7FC0A5A5      # a NaN bit pattern
OUT_CANARY = 0xA5
STATE_CANARY = -77
SOFT_CANARY = 0x7FC05A5A       # a NaN bit pattern around the soft arrays
CTL_KEYS = ("inv_temp", "top_k", "top_p", "plen", "prefix")
CASE = {c.name: c for c in sr.SOFT_CASES}


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


def _con_fields(con, N):
    if con is None:
        return {}
    f = dict(allow_tab=con["tab"].view(np.int32), allow_rows=int(con["rows"]))
    if con["mode"] == "mask":
        f["allow_idx"] = con["idx"].astype(np.int32)
    else:
        f["allow_next"] = con["nxt"].view(np.int16)
        f["allow_start"] = con["start"].astype(np.int32)
        f["allow_state"] = np.full(N + 2, STATE_CANARY, np.int32)
    return f


def _soft_fields(soft):
    """The soft values as the binding's keys: each array between two canary words (the table between two
    canary lines), the pointer past the first."""
    if soft is None:
        return {}
    can = np.array([SOFT_CANARY], np.uint32)
    wrap = lambda a: np.concatenate([can, np.ascontiguousarray(a).view(np.uint32).reshape(-1), can])
    return dict(soft_tab=wrap(soft["tab"]), soft_idx=wrap(soft["idx"].astype(np.int32)), soft_pres=wrap(soft["pres"]),
                soft_freq=wrap(soft["freq"]), soft_rows=int(soft["rows"]))


def _run(ext, d, rf, ctl, fields, probs, ws=None, sync=None, par=0):
    """One launch on the inputs d (controlled when ctl is given; constrained / soft with `fields`) -> the
    buffers check_launch reads, plus allow_state [N + 2] (name 0 at row 1) and the soft arrays as they are
    after the launch."""
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
    held = {}
    if ctl is not None:
        for k in CTL_KEYS:
            held[k] = torch.from_numpy(np.ascontiguousarray(ctl[k])).to(DEV)
            a[k] = held[k].data_ptr()
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            host = v.view(np.int32) if v.dtype == np.uint32 else v
            held[k] = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
            a[k] = held[k].data_ptr() + (4 if k == "allow_state" or k.startswith("soft_") else 0)
        else:
            a[k] = v
    if fields:
        held["con"] = torch.zeros(ext.gen_persist_con_bytes() // 4 + 2, dtype=I32, device=DEV)
        a["con"] = held["con"].data_ptr()
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
    if "allow_state" in held:
        got["allow_state"] = held["allow_state"].cpu().numpy()
    for k in fields:      # the inputs are read only: canaries and values as uploaded
        if k.startswith("soft_") and k in held:
            assert np.array_equal(u32(held[k]), fields[k]), f"{k} was written"
    return got


@functools.lru_cache(maxsize=None)
def _planted(name):
    """The case's inputs, its (possibly moved) controls, its tables, its soft values and the float64
    trajectory: computed once."""
    return sr.case_setup(CASE[name])


def _check(c, d, ctl, con, orc, got, tag="GENSOFT"):
    k = c.ctl
    fails, fig = gr.check_launch(d, orc, got, probs=k.probs, atol=sr.ATOL)
    T = gr.chars_run(orc["alive_after"], k.ML, k.probs)
    print(f"{tag} {c.name:36s} par {got['par']} chars {T}/{k.ML} moved {ctl['moved']} " +
          " ".join(f"{f} {v:9.3e} (atol {sr.ATOL[f]:.2e})" for f, v in fig.items()))
    assert not fails, f"{c.name}: " + "; ".join(fails)
    if con is not None and k.probs:      # exactly 0 outside the set at the last char (a forced one reads no mask)
        free = ctl["plen"] < k.ML
        assert (got["probs"][:k.N][free][~orc["allowed"][k.ML - 1][free]] == 0).all(), c.name
    if con is not None and con["mode"] == "auto":      # the walk's end over the chars the launch ran, against the host walk
        st = got["allow_state"]
        assert st[0] == STATE_CANARY and st[-1] == STATE_CANARY, c.name
        assert np.array_equal(st[1:-1], nr.walk(con, orc["sampled"], T)), c.name


def _launch(ext, c, ws=None, sync=None, par=0):
    k = c.ctl
    assert ext.gen_persist_soft_supported(k.H, k.L, k.V, k.N, k.ML, sr.CON_MODE[c.mode]), c.name
    d, ctl, con, soft, orc = _planted(c.name)
    got = _run(ext, d, orc["rf"], ctl, dict(_con_fields(con, k.N), **_soft_fields(soft)), k.probs, ws, sync, par)
    _check(c, d, ctl, con, orc, got)
    return got


# ---------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("c", sr.CASES_N + sr.CASES_T, ids=lambda c: c.name)
def test_soft_every_name_count_regime(gp, c):
    """H = 256 in each constraint mode: one name, direct, LDS-staged, distributed with two and three name
    tiles; H = 1024, L = 2 (the reference model, at the register cap): the tagged state layout at one name,
    the distributed regime at 17.  Per-name bias lines (the last line in use), penalties of both signs,
    forced prefixes that hold one char twice and three times, a step-0 sample on an empty history."""
    _launch(gp, c)


@pytest.mark.parametrize("c", sr.CASES_A, ids=lambda c: c.name)
def test_soft_every_variant(gp, c):
    """Every supported (H, L) in each constraint mode, at three names."""
    _launch(gp, c)


def test_soft_supported_list(gp):
    for H, L in gr.VARIANTS:
        for m, mode in sr.CON_MODE.items():
            assert gp.gen_persist_soft_supported(H, L, 256, 3, 4, mode) == sr.supported(H, L, m), (H, L, m)
            assert not gp.gen_persist_soft_supported(H, L, 512, 3, 4, mode)      # V = 512 stays on the graph
    assert gp.gen_persist_soft_supported(256, 1, 256, 64, sr.HIST, 0)
    assert not gp.gen_persist_soft_supported(256, 1, 256, 3, sr.HIST + 1, 0)      # the history bounds max_len
    assert not gp.gen_persist_soft_supported(256, 1, 256, 65, 4, 0) and not gp.gen_persist_soft_supported(256, 1, 256, 3, 4, 3)


@pytest.mark.parametrize("c", sr.CASES_G + sr.CASES_GC, ids=lambda c: c.name)
def test_soft_names_that_end(gp, c):
    """Every name has ended after char 1, under both (sos, eos) pairs: with probs set the launch runs every
    char and a dead name counts NULs (with eos = 0 its EOS byte counts as char 0 too); with probs == nullptr
    the launch stops there."""
    _launch(gp, c)


@pytest.mark.parametrize("c", sr.CASES_B + sr.CASES_X, ids=lambda c: c.name)
def test_soft_bias_alone_penalties_alone_and_the_extreme_lines(gp, c):
    """Penalties 0 with a bias (the history walk is skipped), penalties without a bias, and +-1e4 lines on
    the greedy / top_k = 1 names."""
    _launch(gp, c)


@pytest.mark.parametrize("c", sr.CASES_F, ids=lambda c: c.name)
def test_soft_neutral_values_are_the_launch_without_them_bitwise(gp, c):
    """Line 0 (all zero) and penalties 0 through the SOFT instantiation: every output byte, probability and
    workspace word of the controlled / constrained launch without soft keys, in each constraint mode."""
    d, ctl, con, soft, orc = _planted(c.name)
    assert not soft["idx"].any() and not soft["pres"].any() and not soft["freq"].any() and not soft["tab"][0].any()
    plain = _run(gp, d, orc["rf"], ctl, _con_fields(con, c.ctl.N), True)
    got = _run(gp, d, orc["rf"], ctl, dict(_con_fields(con, c.ctl.N), **_soft_fields(soft)), True)
    _check(c, d, ctl, con, orc, got)
    for k in ("out", "err", "sync", "ws_before", "ws_after") + (("allow_state",) if c.mode == "auto" else ()):
        assert np.array_equal(plain[k], got[k]), k
    assert np.array_equal(plain["probs"].view(np.uint32), got["probs"].view(np.uint32))


@pytest.mark.parametrize("name", ["none-n-N9", "none-n-N17", "auto-n-N17"])
def test_soft_an_out_of_range_line_is_flagged_and_taken_as_line_0(gp, name):
    """One line index far outside the table: err[0] & 16, err[1] the value, err[2] the name; the launch
    completes, and everything it computed is the trajectory with line 0 for that name."""
    c = CASE[name]
    d, ctl, con, soft, orc = _planted(name)
    bad, n, value = sr.with_oob(soft, ctl)
    ctl, orc = sr.plant(d, sr.controls(c), con, bad, cr.case_plan(c.ctl))      # the uniforms planted on line 0's values
    assert orc["soft_oob"].sum() == 1 and orc["soft_oob"][n]
    got = _run(gp, d, orc["rf"], ctl, dict(_con_fields(con, c.ctl.N), **_soft_fields(bad)), True)
    err = got["err"]
    assert err[0] == 16 and err[1] == value and err[2] == n, err
    got["err"] = np.zeros_like(err)
    _check(c, d, ctl, con, orc, got, "GENSOFT-OOB")


@pytest.mark.parametrize("name", ["none-n-N9", "mask-n-N17", "auto-n-N8"])
def test_soft_rows_are_sample_ctl_s_on_the_launch_s_logits(gp, name):
    """The per-char graph's sampler (ext.sample_ctl with the soft keys) driven char by char on the logits the
    launch left in its workspace, its own output row as the history: byte-identical rows."""
    c = CASE[name]
    k = c.ctl
    d, ctl, con, soft, orc = _planted(name)
    got = _launch(gp, c)
    T = gr.chars_run(orc["alive_after"], k.ML, k.probs)
    dec = gr.ws_decode(got["ws_after"], got["par"], k.H, k.L, k.V, k.ML, k.N, T)
    N, V, ML = k.N, k.V, k.ML
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    held = {x: up(ctl[x]) for x in CTL_KEYS}
    sheld = dict(tab=up(soft["tab"]), idx=up(soft["idx"].astype(np.int32)), pres=up(soft["pres"]), freq=up(soft["freq"]))
    ids = torch.zeros(N, dtype=I32, device=DEV)
    alive = torch.ones(N, dtype=I32, device=DEV)
    out = torch.zeros(N, ML + 1, dtype=torch.uint8, device=DEV)
    err = torch.zeros(4, dtype=I32, device=DEV)
    rfd = up(orc["rf"])
    extra = {}
    if con is not None:
        extra = dict(allow_tab=up(con["tab"].view(np.int32)), allow_rows=int(con["rows"]))
        if con["mode"] == "mask":
            extra["allow_idx"] = up(con["idx"].astype(np.int32))
        else:
            extra["allow_next"] = up(con["nxt"].view(np.int16))
            extra["allow_state"] = up(con["start"].astype(np.int32))
    for t in range(T):
        lg = up(dec["logits"][t][:N].astype(np.float32))
        a = dict(logits=lg.data_ptr(), rf=rfd.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(), alive=alive.data_ptr(),
                 N=N, V=V, step=t, max_len=ML, eos=k.eos, err=err.data_ptr(), soft_tab=sheld["tab"].data_ptr(),
                 soft_idx=sheld["idx"].data_ptr(), soft_rows=int(soft["rows"]), soft_pres=sheld["pres"].data_ptr(),
                 soft_freq=sheld["freq"].data_ptr(), **{x: held[x].data_ptr() for x in CTL_KEYS},
                 **{x: (v if isinstance(v, int) else v.data_ptr()) for x, v in extra.items()})
        gp.sample_ctl(a, S())
    torch.cuda.synchronize()
    assert not u32(err).any()
    assert np.array_equal(out.cpu().numpy()[:, :T], got["out"][:N, :T]), name


def test_soft_launches_alternate_with_the_others_on_one_workspace(gp):
    """Parity 0, 1, 0, 1 on one workspace: soft, controlled, soft + automaton, soft + per-position."""
    H, L, V, ML = 256, 1, 256, 4
    ws, sync = _new_ws(gp, H, L, V, ML)
    _launch(gp, CASE["none-n-N9"], ws, sync, 0)
    c = cr.CtlCase("alt-ctl-N8", H, L, V, 8, ML, 7, 3, off=2)
    d = cr.case_inputs(c)
    ctl, orc = cr.plant(d, cr.controls(c))
    fails, _ = gr.check_launch(d, orc, _run(gp, d, orc["rf"], ctl, {}, True, ws, sync, 1), atol=cr.ATOL)
    assert not fails, fails
    _launch(gp, CASE["auto-n-N17"], ws, sync, 0)
    _launch(gp, CASE["mask-n-N8"], ws, sync, 1)


def test_soft_binding_rejects_inconsistent_field_sets(gp):
    c = CASE["none-n-N8"]
    d, ctl, con, soft, orc = _planted(c.name)
    f = _soft_fields(soft)
    bad = [{k: v for k, v in f.items() if k != drop} for drop in ("soft_tab", "soft_idx", "soft_pres", "soft_freq")]
    bad.append(dict(f, soft_rows=0))
    for b in bad:
        with pytest.raises(RuntimeError):
            _run(gp, d, orc["rf"], ctl, b, True)
    with pytest.raises(RuntimeError):                             # soft controls without the five controls
        _run(gp, d, orc["rf"], None, f, True)

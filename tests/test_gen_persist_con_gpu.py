"""Constraints inside the controlled persistent small-batch launch (gen_persist_con.hip, docs/DESIGN.md
§4e / §4g), kernel level.

As tests/test_gen_persist_ctl_gpu.py: ``ext.gen_persist`` with the five control arrays and the constraint
fields on a caller-owned, pre-filled workspace, canary-filled ``out`` / ``probs`` / ``allow_state``, every
state, logit, id, row and probability checked by gen_ref.check_launch against the float64 CONSTRAINED
trajectory of models/gen_con_ref.py (which plants the uniforms inside the sets and keeps the kept sets
clear of fp32 rounding; tests/test_gen_con_ref.py shows the checker to fail on every planted defect).
Both modes -- per-position table and automaton -- run on every case.
"""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import gen_con_ref as nr
from gru_mpi_cuda_amd.models import gen_ctl_ref as cr
from gru_mpi_cuda_amd.models import gen_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32 = torch.int32
PROBS_CANARY = 0x7FC0A5A5      # a NaN bit pattern
OUT_CANARY = 0xA5
STATE_CANARY = -77
CTL_KEYS = ("inv_temp", "top_k", "top_p", "plen", "prefix")
MODE = {"mask": 1, "auto": 2}
CASE = {c.name: c for c in nr.CON_CASES}


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
    """The constraint as the binding's fields: numpy arrays (uploaded by _run) and allow_rows."""
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


def _run(ext, d, rf, ctl, fields, probs, ws=None, sync=None, par=0):
    """One launch on the inputs d (controlled when ctl is given, constrained with `fields`) -> the buffers
    check_launch reads, plus allow_state [N + 2] (name 0 at row 1: a canary row on either side)."""
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
            held[k] = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
            a[k] = held[k].data_ptr() + (4 if k == "allow_state" else 0)      # name 0 at row 1
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
    return got


@functools.lru_cache(maxsize=None)
def _planted(name):
    """The case's inputs, its (possibly moved) controls, its tables and the float64 trajectory: computed once."""
    return nr.case_setup(CASE[name])


def _check(c, d, ctl, con, orc, got, tag="GENCON"):
    k = c.ctl
    fails, fig = gr.check_launch(d, orc, got, probs=k.probs, atol=nr.ATOL)
    T = gr.chars_run(orc["alive_after"], k.ML, k.probs)
    print(f"{tag} {c.name:32s} par {got['par']} chars {T}/{k.ML} moved {ctl['moved']} " +
          " ".join(f"{f} {v:9.3e} (atol {nr.ATOL[f]:.2e})" for f, v in fig.items()))
    assert not fails, f"{c.name}: " + "; ".join(fails)
    if k.probs:      # exactly 0 outside the set at the last char (a forced one reads no mask)
        free = ctl["plen"] < k.ML
        assert (got["probs"][:k.N][free][~orc["allowed"][k.ML - 1][free]] == 0).all(), c.name
    if con["mode"] == "auto":      # the walk's end over the chars the launch ran, and the rows around it
        st = got["allow_state"]
        assert st[0] == STATE_CANARY and st[-1] == STATE_CANARY, c.name
        assert np.array_equal(st[1:-1], nr.walk(con, orc["sampled"], T)), c.name


def _launch(ext, c, ws=None, sync=None, par=0):
    k = c.ctl
    assert ext.gen_persist_con_supported(k.H, k.L, k.V, k.N, k.ML, MODE[c.mode]), c.name
    d, ctl, con, orc = _planted(c.name)
    got = _run(ext, d, orc["rf"], ctl, _con_fields(con, k.N), k.probs, ws, sync, par)
    _check(c, d, ctl, con, orc, got)
    return got


# ---------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("c", nr.CASES_N + nr.CASES_T, ids=lambda c: c.name)
def test_con_every_name_count_regime(gp, c):
    """H = 256: one name, direct, LDS-staged, distributed with two and three name tiles; H = 1024, L = 2
    (the reference model, the variant at the register cap): the tagged state layout at one name, the
    distributed regime at 17.  Tables: the last line / state in use, one-char sets under every control
    mixture, top_k beyond the set, the BEYOND uniform, prefix bytes outside their sets."""
    _launch(gp, c)


@pytest.mark.parametrize("c", nr.CASES_V, ids=lambda c: c.name)
def test_con_vocab_512(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", nr.CASES_A + nr.CASES_A512, ids=lambda c: c.name)
def test_con_every_variant(gp, c):
    """Every variant of the controlled launch has a constrained one in both modes (ten at V = 256, eight
    at V = 512)."""
    k = c.ctl
    assert gp.gen_persist_ctl_supported(k.H, k.L, k.V, k.N, k.ML)
    _launch(gp, c)


def test_con_unsupported_shapes_are_the_controlled_launch_s(gp):
    for H, L in gr.VARIANTS:
        for V in (256, 512):
            for mode in (1, 2):
                assert gp.gen_persist_con_supported(H, L, V, 3, 4, mode) == gp.gen_persist_ctl_supported(H, L, V, 3, 4)
    assert not gp.gen_persist_con_supported(256, 1, 256, 3, 4, 0) and not gp.gen_persist_con_supported(256, 1, 256, 65, 4, 1)


@pytest.mark.parametrize("c", nr.CASES_G, ids=lambda c: c.name)
def test_con_names_that_end(gp, c):
    """Every name has ended after char 1, half of them by an EOS byte inside a prefix of full length, half
    mid-way by a sampled EOS (the state then follows nxt[q][eos] = 0); with probs == nullptr the launch
    stops there and allow_state holds the walk over the chars it ran."""
    _launch(gp, c)


@pytest.mark.parametrize("c", nr.CASES_F, ids=lambda c: c.name)
def test_con_a_free_table_is_the_controlled_launch_bitwise(gp, c):
    """A line-0-only table / a one-state free automaton: every output byte, probability and workspace word
    of the unconstrained controlled launch."""
    d, ctl, con, orc = _planted(c.name)
    plain = _run(gp, d, orc["rf"], ctl, {}, True)
    got = _run(gp, d, orc["rf"], ctl, _con_fields(con, c.ctl.N), True)
    _check(c, d, ctl, con, orc, got)
    for k in ("out", "err", "sync", "ws_before", "ws_after"):
        assert np.array_equal(plain[k], got[k]), k
    assert np.array_equal(plain["probs"].view(np.uint32), got["probs"].view(np.uint32))


@pytest.mark.parametrize("name", ["mask-n-N9", "auto-n-N9", "mask-n-N17", "auto-n-N17"])
def test_con_an_out_of_range_line_is_flagged_and_taken_as_line_0(gp, name):
    """One idx entry / one start state far outside the table: err[0] & 16, err[1] the value, err[2] the
    name; the launch completes, and everything it computed is the trajectory with line 0 there (the walk
    continuing from state 0)."""
    c = CASE[name]
    d, ctl, con, orc = _planted(name)
    bad, n, value = nr.with_oob(c, con, ctl)
    ctl, orc = nr.plant(d, cr.controls(c.ctl), bad, cr.case_plan(c.ctl))      # the uniforms planted on line 0's sets
    assert orc["oob"].sum() == 1 and orc["oob"][0, n] and orc["line"][0, n] == 0
    got = _run(gp, d, orc["rf"], ctl, _con_fields(bad, c.ctl.N), True)
    err = got["err"]
    assert err[0] == 16 and err[1] == value and err[2] == n, err
    got["err"] = np.zeros_like(err)
    _check(c, d, ctl, bad, orc, got, "GENCON-OOB")


def test_con_plain_controlled_and_constrained_launches_alternate_on_one_workspace(gp):
    """Parity 0, 1, 0, 1, 0 on one workspace: plain, per-position, controlled, automaton, per-position."""
    H, L, V, ML = 256, 1, 256, 4
    ws, sync = _new_ws(gp, H, L, V, ML)
    p0 = gr.Case("alt-plain-N16", H, L, V, 16, ML, 7, 3, seed_off=10)
    d = gr.case_inputs(p0)
    orc = gr.plant_uniforms(d)
    fails, _ = gr.check_launch(d, orc, _run(gp, d, orc["rf"], None, {}, True, ws, sync, 0))
    assert not fails, fails
    _launch(gp, CASE["mask-n-N9"], ws, sync, 1)
    c = cr.CtlCase("alt-ctl-N8", H, L, V, 8, ML, 7, 3, off=2)
    d = cr.case_inputs(c)
    ctl, orc = cr.plant(d, cr.controls(c))
    fails, _ = gr.check_launch(d, orc, _run(gp, d, orc["rf"], ctl, {}, True, ws, sync, 0), atol=cr.ATOL)
    assert not fails, fails
    _launch(gp, CASE["auto-n-N17"], ws, sync, 1)
    _launch(gp, CASE["mask-n-N8"], ws, sync, 0)


def test_con_binding_rejects_inconsistent_field_sets(gp):
    c = CASE["mask-n-N8"]
    d, ctl, con, orc = _planted(c.name)
    m = _con_fields(con, c.ctl.N)
    a = _con_fields(_planted("auto-n-N8")[2], c.ctl.N)
    bad = [
        {k: v for k, v in m.items() if k != "allow_idx"},         # a table alone
        {k: v for k, v in m.items() if k != "allow_tab"},         # idx alone
        dict(m, allow_rows=0),
        dict(a, allow_idx=m["allow_idx"]),                        # idx with an automaton
        {k: v for k, v in a.items() if k != "allow_start"},
        {k: v for k, v in a.items() if k != "allow_next"},
        {k: v for k, v in a.items() if k != "allow_tab"},
        dict(a, allow_rows=65536),
        dict(a, allow_rows=0),
        dict(m, allow_state=a["allow_state"]),                    # a state array without an automaton
    ]
    for f in bad:
        with pytest.raises(RuntimeError):
            _run(gp, d, orc["rf"], ctl, f, True)
    with pytest.raises(RuntimeError):                             # constraints without the controls
        _run(gp, d, orc["rf"], None, m, True)

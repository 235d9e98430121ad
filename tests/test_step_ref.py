"""The per-element reference of the step kernels and the two-layer wavefront (models/step_ref.py),
pinned down on the CPU before any GPU run: with the operand rounding off it equals torch.autograd,
the tolerances the GPU tests import are the measured emulator-vs-reference deviations, and every
planted bug fails them."""
import pytest
import torch

from gru_mpi_cuda_amd.models import seq_ref as sr
from gru_mpi_cuda_amd.models import step_ref as st

F64 = torch.float64


def _R(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=F64)


# ------------------------------------------------------------------------------ the reference is right
@pytest.mark.parametrize("mode", ["table", "gi", "fused"])
def test_step_refs_equal_autograd(mode):
    """exact=True: fwd_step_ref is a one-step GRU, and bwd_step_ref fed with its saves returns the
    gradients torch.autograd gives for the loss sum(dy h) + sum(dgh_next (h Whh^T)) + sum(carry_in h),
    i.e. for a dh of dy + dgh_next . Whh + carry_in: d/dGi = dgi, d/d(gh) = dgh, the direct path
    d/dh_prev = carry_out."""
    H, Bp, V, Kin = 32, 8, 16, 24
    R = _R(7)
    Whh, bhh, hp = R(3 * H, H) * H ** -0.5, R(3 * H) * 0.1, R(Bp, H) * 0.5
    P, ids, Gi = R(V, 3 * H) * 0.5, torch.randint(0, V, (Bp,), dtype=torch.int32), R(Bp, 3 * H) * 0.5
    x, Wih, bih = R(Bp, Kin), R(3 * H, Kin) * Kin ** -0.5, R(3 * H) * 0.1
    dy, dgn, cin = R(Bp, H), R(Bp, 3 * H), R(Bp, H)
    kw = dict(table=dict(P=P, ids=ids), gi=dict(Gi=Gi), fused=dict(x=x, Wih=Wih, bih=bih))[mode]
    f = st.fwd_step_ref(Whh, bhh, hp, exact=True, **kw)
    b = st.bwd_step_ref(dy, f["r"], f["z"], f["n"], f["ghn"], hp, Whh, dgh_next=dgn, carry_in=cin, exact=True)
    # autograd: gi and gh as leaves, the blend operand as its own leaf (the direct path of h_prev)
    gi0 = P[ids.long()] if mode == "table" else Gi if mode == "gi" else x @ Wih.T + bih
    gi = gi0.clone().requires_grad_(True)
    gh = (hp @ Whh.T + bhh).clone().requires_grad_(True)
    hb = hp.clone().requires_grad_(True)
    h, r, z, n, ghn = sr._gates(gi, gh, hb)
    tol = dict(rtol=1e-12, atol=1e-13)
    for k, v in zip(("h", "r", "z", "n", "ghn"), (h, r, z, n, ghn)):
        torch.testing.assert_close(f[k], v.detach(), **tol)
    ((dy + dgn @ Whh + cin) * h).sum().backward()
    torch.testing.assert_close(b["dgi"], gi.grad, **tol)
    torch.testing.assert_close(b["dgh"], gh.grad, **tol)
    torch.testing.assert_close(b["carry_out"], hb.grad, **tol)
    # first step: no product, no carry
    b0 = st.bwd_step_ref(dy, f["r"], f["z"], f["n"], f["ghn"], hp, Whh, exact=True)
    gi.grad = gh.grad = hb.grad = None
    (dy * sr._gates(gi, gh, hb)[0]).sum().backward()
    torch.testing.assert_close(b0["dgi"], gi.grad, **tol)
    torch.testing.assert_close(b0["carry_out"], hb.grad, **tol)


@pytest.mark.parametrize("mode,h0", [("ids", "both"), ("gi", "none"), ("ids", "lo"), ("gi", "hi")])
def test_wave_ref_equals_a_two_layer_gru(mode, h0):
    """exact=True: wave_ref equals torch.nn.GRU(num_layers=2) in float64 (same gate order r, z, n)."""
    H, Bp, T, V = 32, 8, 5, 16
    R = _R(11)
    d = dict(Whh_lo=R(3 * H, H) * H ** -0.5, Wih_hi=R(3 * H, H) * H ** -0.5, Whh_hi=R(3 * H, H) * H ** -0.5,
             bhh_lo=R(3 * H) * 0.1, bih_hi=R(3 * H) * 0.1, bhh_hi=R(3 * H) * 0.1, P=R(V, 3 * H) * 0.5,
             ids=torch.randint(0, V, (T, Bp), dtype=torch.int32), Gi=R(T, Bp, 3 * H) * 0.5,
             h0_lo=R(Bp, H) * 0.5, h0_hi=R(Bp, H) * 0.5)
    o = st.wave_ref(exact=True, **st.wave_kw(d, T, Bp, mode, h0))
    # nn.GRU with an identity layer-0 input projection: its input IS lo's Gi
    gru = torch.nn.GRU(3 * H, H, num_layers=2).to(F64)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H, dtype=F64)); gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(d["Whh_lo"]); gru.bias_hh_l0.copy_(d["bhh_lo"])
        gru.weight_ih_l1.copy_(d["Wih_hi"]); gru.bias_ih_l1.copy_(d["bih_hi"])
        gru.weight_hh_l1.copy_(d["Whh_hi"]); gru.bias_hh_l1.copy_(d["bhh_hi"])
        gi = d["P"][d["ids"].long()] if mode == "ids" else d["Gi"]
        zero = torch.zeros(Bp, H, dtype=F64)
        h0s = torch.stack([d["h0_lo"] if h0 in ("lo", "both") else zero, d["h0_hi"] if h0 in ("hi", "both") else zero])
        y, hn = gru(gi, h0s)
    torch.testing.assert_close(o["hi"]["HS"][1:], y, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(o["lo"]["HS"][-1], hn[0], rtol=1e-11, atol=1e-12)
    assert torch.equal(o["hi"]["HS"][0], h0s[1]) and torch.equal(o["lo"]["HS"][0], h0s[0])


def test_references_round_only_the_mfma_operands():
    """The blend takes the fp32 h_prev: a reference that rounded it would differ by up to 2^-9 |h|."""
    d = st.fwd_step_inputs(64, 32, 64, seed=0)
    a = st.fwd_step_ref(d["Whh"], d["bhh"], d["hprev"], Gi=d["Gi"])
    b = st.fwd_step_ref(d["Whh"], d["bhh"], sr.bf16_round(d["hprev"]), Gi=d["Gi"])
    assert torch.equal(a["r"], b["r"]) and torch.equal(a["ghn"], b["ghn"]) and not torch.equal(a["h"], b["h"])


# ------------------------------------------------------------------------------ tolerances are measured
def test_tolerances_derive_from_measurement():
    for fam, dev in {**st.MEASURED_DEV, **st.WAVE_MEASURED_DEV}.items():
        assert dev > 0 and st.ATOL[fam] == 4.0 * dev
    assert st.RTOL["bf16_grad"] == sr.RTOL["bf16_grad"] == 2.0 ** -7
    assert st.RTOL["f32_state"] == st.RTOL["f32_carry"] == st.RTOL["wave_f32_state"] == 0.0
    # the wavefront has a family of its own because it exceeds seq_ref's figure; hi inherits lo's flips
    assert sr.MEASURED_DEV["f32_state"] < st.WAVE_MEASURED_LO <= st.WAVE_MEASURED_DEV["wave_f32_state"]
    assert sr.MEASURED_DEV["f32_state"] == 1.36e-03, "seq_ref's figures are not enlarged"


def test_recorded_deviations_cover_a_fresh_measurement():
    """Re-measure the quick shapes (H <= 512, Bp <= 256, one seed): nothing exceeds the recorded
    maxima, and the recorded maxima are of the same order (not padded by hand)."""
    quick = lambda c: c[1] <= 512 and c[2] <= 256
    got = st.measure_deviations(seeds=(1,), fwd_cases=[c for c in st.FWD_STEP_CASES if quick(c)],
                                bwd_cases=[c for c in st.BWD_STEP_CASES if quick(c)],
                                wave_shapes=[s for s in st.WAVE_SHAPES if s[0] <= 512])
    rec = {**st.MEASURED_DEV, **st.WAVE_MEASURED_DEV}
    print({k: f"{v:.3e}" for k, v in got.items()}, rec)
    for fam, r in rec.items():
        assert r / 16 <= got[fam] <= r, (fam, got[fam])
    assert got["wave_lo_f32_state"] <= st.WAVE_MEASURED_LO


# ------------------------------------------------------------------------------ the tolerances bite
def _bad(pairs):
    return {k for k, fam, a, b in pairs if st.mismatch(a, b, fam) is not None}


FWD_MUT_SHAPES = [(128, 32, "gi", 0), (512, 96, "table", 0), (320, 256, "fused", 64), (256, 128, "fused", 256)]
BWD_MUT_SHAPES = [(128, 32), (320, 256)]
WAVE_MUT_SHAPES = [(256, 64, 9, "ids", "both"), (512, 96, 2, "gi", "none")]

# which outputs must notice each planted bug
MUT_SEEN_IN = {
    "fwd_b_hn_added_outside_r": ("h", "n"),
    "fwd_k_fragment_dropped": ("h", "r", "z", "n", "ghn"),
    "fwd_blend_from_bf16_h_prev": ("h",),
    "fwd_fused_n_parts_summed_before_r": ("h", "n"),
    "fwd_r_and_z_saves_swapped": ("r", "z"),
    "bwd_dgh_n_row_without_r": ("dgh",),
    "bwd_carry_out_without_product": ("carry_out",),
    "bwd_daz_with_z_for_one_minus_z": ("dgh", "dgi"),
    "wave_hi_reads_h_lo_one_step_stale": ("hi.HS", "hi.r", "hi.z", "hi.n"),
    "wave_hi_b_ih_dropped": ("hi.HS", "hi.r", "hi.z", "hi.n"),
    "wave_hi_r_gate_without_input_part": ("hi.HS", "hi.r"),
}


def _mut_cases():
    for name, (kind, mut) in sorted(st.MUTATIONS.items()):
        if kind in ("fwd", "fwd_fused"):
            for c in FWD_MUT_SHAPES:
                if kind == "fwd" or c[2] == "fused":
                    yield name, kind, mut, c
        elif kind == "bwd":
            for c in BWD_MUT_SHAPES:
                yield name, kind, mut, c
        else:
            for c in WAVE_MUT_SHAPES:
                yield name, kind, mut, c


def _run(kind, mut, c):
    if kind in ("fwd", "fwd_fused"):
        return _bad(st.step_pairs(*st.fwd_step_case(*c, seed=3, mut=mut), st._FWD_FAMILY))
    if kind == "bwd":
        return _bad(st.step_pairs(*st.bwd_step_case(*c, first=False, seed=3, mut=mut), st._BWD_FAMILY))
    return _bad(st.wave_pairs(*st.wave_case(*c, seed=3, mut=mut)))


@pytest.mark.parametrize("kind,c", [("fwd", c) for c in FWD_MUT_SHAPES] + [("bwd", c) for c in BWD_MUT_SHAPES] +
                         [("wave", c) for c in WAVE_MUT_SHAPES])
def test_correct_emulation_passes(kind, c):
    assert _run(kind, None, c) == set()
    if kind == "bwd":   # the first step too
        assert _bad(st.step_pairs(*st.bwd_step_case(*c, first=True, seed=3), st._BWD_FAMILY)) == set()


@pytest.mark.parametrize("name,kind,mut,c", list(_mut_cases()))
def test_planted_bug_fails_the_tolerances(name, kind, mut, c):
    bad = _run(kind, mut, c)
    for k in MUT_SEEN_IN[name]:
        assert k in bad, f"{name} went unnoticed in {k} (noticed in {sorted(bad)})"


def test_every_listed_mutation_is_planted():
    assert set(MUT_SEEN_IN) == set(st.MUTATIONS) and len(st.MUTATIONS) == 11


def test_case_tables_cover_every_launchable_kernel():
    assert {c[0] for c in st.FWD_STEP_CASES} == {"reg", "lds64", "lds128", "big"}
    assert {c[0] for c in st.BWD_STEP_CASES} == {"reg", "lds8", "sk2", "sk4"}
    assert {c[3] for c in st.FWD_STEP_CASES if c[0] == "reg"} == {"table", "gi", "fused"}

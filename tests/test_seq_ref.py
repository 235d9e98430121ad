"""The per-element reference of the persistent sequence kernels (models/seq_ref.py), pinned down on
the CPU before any GPU run: the float64 BPTT equals torch.autograd, the tolerances the GPU tests
import are the measured emulator-vs-reference deviations, and every planted bug fails them."""
import pytest
import torch

from gru_mpi_cuda_amd.models import seq_ref as sr


# ------------------------------------------------------------------------------ the reference is right
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("mode", ["gi", "ids"])
def test_bwd_ref_equals_autograd(T, mode):
    """Rounding off, bwd_ref fed with fwd_ref's saves is plain BPTT: dW_hh, db_hh, dGi (dP for the
    table input) and dh0 equal torch.autograd of the float64 forward to 1e-10 relative."""
    H, Bp, V = 32, 8, 16
    g = torch.Generator().manual_seed(T)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Whh, bhh, h0 = R(3 * H, H) * H ** -0.5, R(3 * H) * 0.1, R(Bp, H) * 0.5
    Gi, P = R(T, Bp, 3 * H) * 0.5, R(V, 3 * H) * 0.5
    ids = torch.randint(0, V, (T, Bp), generator=g, dtype=torch.int32)
    dy = R(T, Bp, H)
    kw = dict(Gi=Gi) if mode == "gi" else dict(P=P, ids=ids)
    f = sr.fwd_ref(Whh, bhh, T, Bp, h0=h0, exact=True, **kw)
    b = sr.bwd_ref(dy, f["r"], f["z"], f["n"], f["ghn"], f["HS"], Whh, ids=ids if mode == "ids" else None, V=V,
                   rows=Bp, exact=True)
    leaves = [t.clone().requires_grad_(True) for t in (Whh, bhh, h0, Gi, P)]
    W_, b_, h_, Gi_, P_ = leaves
    h, loss = h_, 0.0
    for t in range(T):
        gi = Gi_[t] if mode == "gi" else P_[ids[t].long()]
        h = sr._gates(gi, h @ W_.T + b_, h)[0]
        loss = loss + (dy[t] * h).sum()
    loss.backward()
    tol = dict(rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dWhh_part"].sum(0), W_.grad, **tol)
    torch.testing.assert_close(b["dbhh_part"].sum(0), b_.grad, **tol)
    torch.testing.assert_close(b["dh0"], h_.grad, **tol)
    if mode == "gi":
        torch.testing.assert_close(b["dgi"], Gi_.grad, **tol)
    else:
        torch.testing.assert_close(b["dP_part"].sum(0), P_.grad, **tol)
    # the input-side bias gradient is the column sum of dGi
    torch.testing.assert_close(b["dbih_part"].sum(0), b["dgi"].sum((0, 1)), **tol)
    # forward: HS[0] is h0 and the saves reproduce the state
    assert torch.equal(f["HS"][0], h0)
    torch.testing.assert_close(f["HS"][1:], f["n"] + f["z"] * (f["HS"][:-1] - f["n"]), **tol)


def test_fused_dy_is_dl_times_wfc():
    d = sr.bwd_inputs(64, 32, 2, seed=0)
    args = (d["r"], d["z"], d["n"], d["ghn"], d["HS"], d["Whh"])
    a = sr.bwd_ref(None, *args, dl=d["dl"], Wfc=d["Wfc"])
    dy = (d["dl"].double() @ d["Wfc"].double()).reshape(2, 32, 64)
    b = sr.bwd_ref(dy, *args)
    assert torch.equal(a["dgi"], b["dgi"]) and torch.equal(a["dWhh_part"], b["dWhh_part"])


def test_partials_are_per_row_block():
    """Row-block partials are the reference restricted to that block's rows, for 32- and 16-row blocks."""
    d = sr.bwd_inputs(64, 64, 3, seed=1)
    args = (d["dy"], d["r"], d["z"], d["n"], d["ghn"], d["HS"], d["Whh"])
    full = sr.bwd_ref(*args, ids=d["ids"], V=256, rows=64)
    for rows in (32, 16):
        p = sr.bwd_ref(*args, ids=d["ids"], V=256, rows=rows)
        assert p["dbhh_part"].shape == (64 // rows, 192)
        for k in ("dbhh_part", "dbih_part", "dWhh_part", "dP_part"):
            torch.testing.assert_close(p[k].sum(0), full[k][0], rtol=1e-12, atol=1e-14)
        blk = p["dgh"][:, rows:2 * rows].sum((0, 1))
        torch.testing.assert_close(p["dbhh_part"][1], blk, rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------ layout decoders
def test_hf_layout_matches_kernels_h():
    """Element by element against the address formula documented at SeqFwdArgs::HF."""
    T1, Bp, H = 2, 64, 48
    HS = torch.arange(T1 * Bp * H, dtype=torch.float32).reshape(T1, Bp, H)
    HF = sr.hf_encode(HS)
    nunit, nrb = H // 16, Bp // 32
    for t, u, rb, l, e in [(0, 0, 0, 0, 0), (1, 2, 1, 63, 7), (1, 1, 0, 17, 3), (0, 2, 1, 40, 5)]:
        got = HF[((t * nunit + u) * nrb + rb) * 512 + l * 8 + e]
        assert got == HS[t, 32 * rb + 8 * (l >> 4) + e, 16 * u + (l & 15)]
    assert torch.equal(sr.hf_decode(HF, T1, Bp, H), HS)


def test_s16_and_transposed_layouts():
    T, Bp, H = 2, 32, 16
    g = torch.Generator().manual_seed(0)
    r, z, n, gh = (torch.randn(T, Bp, H, generator=g) for _ in range(4))
    s = sr.s16_encode(r, z, n, gh)
    assert s.shape == (T, Bp, H, 4) and s.dtype == torch.bfloat16
    w = s.view(torch.int16).to(torch.int32) & 0xFFFF            # st_save16: word0 = r | z << 16, word1 = n | gh_n << 16
    bits = lambda x: x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(w[..., 0] | (w[..., 1] << 16), bits(r) | (bits(z) << 16))
    assert torch.equal(w[..., 2] | (w[..., 3] << 16), bits(n) | (bits(gh) << 16))
    for got, ref in zip(sr.s16_decode(s), (r, z, n, gh)):
        assert torch.equal(got, ref.to(torch.bfloat16))
    X = torch.randn(T, Bp, 3 * H, generator=g)
    XT = sr.ht_encode(X, T * Bp + 64)
    assert XT.shape == (3 * H, T * Bp + 64) and torch.isnan(XT[:, T * Bp:]).all()
    assert XT[5, 1 * Bp + 3] == X[1, 3, 5]                      # step t at column t * Bp + b
    assert torch.equal(sr.ht_decode(XT, T, Bp), X)


# ------------------------------------------------------------------------------ tolerances are measured
def test_tolerances_derive_from_measurement():
    for fam, dev in sr.MEASURED_DEV.items():
        assert dev > 0 and sr.ATOL[fam] == 4.0 * dev
    assert sr.RTOL["bf16_copy"] == sr.RTOL["bf16_grad"] == 2.0 ** -7
    assert sr.RTOL["f32_state"] <= 1e-4 and sr.RTOL["f32_part"] <= 1e-4


def test_recorded_deviations_cover_a_fresh_measurement():
    """Re-measure |emulate - ref| on the quick GPU shapes (H <= 512, one seed); nothing may exceed the
    recorded maxima, and the recorded maxima are of the same order (not padded by hand)."""
    got = sr.measure_deviations(seeds=(1,), fwd_shapes=[s for s in sr.FWD_SHAPES if s[0] <= 512],
                                bwd_shapes=[s for s in sr.BWD_SHAPES if s[0] <= 512])
    print({k: f"{v:.3e}" for k, v in got.items()}, sr.MEASURED_DEV)
    for fam, rec in sr.MEASURED_DEV.items():
        assert rec / 8 <= got[fam] <= rec, (fam, got[fam])
        assert got[fam + "_raw"] <= sr.MEASURED_RAW[fam], (fam, got[fam + "_raw"])


# ------------------------------------------------------------------------------ the tolerances bite
def _mismatches(pairs):
    return {k: m for k, fam, a, b in pairs if (m := sr.mismatch(a, b, fam)) is not None}


MUT_SHAPES = [(256, 64, 7), (512, 256, 7)]    # both workgroup mappings (Bp/32 % 8 != 0 and == 0)


@pytest.mark.parametrize("H,Bp,T", MUT_SHAPES)
def test_correct_emulation_passes(H, Bp, T):
    emu, ref = sr.bwd_case(H, Bp, T, seed=3, xring=2, fuse_w=True)
    assert _mismatches(sr.bwd_pairs(emu, ref)) == {}
    d = sr.fwd_inputs(H, Bp, T, seed=3)
    ref = sr.fwd_ref(d["Whh"], d["bhh"], T, Bp, P=d["P"], ids=d["ids"], h0=d["h0"])
    emu = sr.emulate_fwd(d["Whh"], d["bhh"], T, Bp, P=d["P"], ids=d["ids"], h0=d["h0"], xring=4)
    assert _mismatches(sr.fwd_pairs(emu, ref)) == {}


# which outputs must notice each planted bug
MUT_SEEN_IN = {
    "a_stale_exchange_slot_one_row_block": ("dgi",),
    "b_ring_slot_reused_one_step_early": ("dgi",),
    "c_carry_dropped_at_one_step": ("dgi",),
    "d_row_block_missing_from_partials": ("dbhh_part", "dbih_part", "dP_part"),
    "e_dgi_n_rows_hold_dan_r": ("dgi", "dbih_part", "dP_part"),
    "f_dwhh_skips_last_step": ("dWhh_part",),
    "g_fwd_tile_reads_h_two_steps_back": ("HS", "HSb"),
    "h_fwd_h0_left_out_of_step_0": ("HS", "HSb"),
}


@pytest.mark.parametrize("name", sorted(sr.MUTATIONS))
@pytest.mark.parametrize("H,Bp,T", MUT_SHAPES)
def test_planted_bug_fails_the_tolerances(H, Bp, T, name):
    direction, build = sr.MUTATIONS[name]
    mut = build(T, Bp, H)
    if direction == "bwd":
        emu, ref = sr.bwd_case(H, Bp, T, seed=3, xring=2, fuse_w=True, mut=mut)
        bad = _mismatches(sr.bwd_pairs(emu, ref))
    else:
        d = sr.fwd_inputs(H, Bp, T, seed=3)
        ref = sr.fwd_ref(d["Whh"], d["bhh"], T, Bp, P=d["P"], ids=d["ids"], h0=d["h0"])
        emu = sr.emulate_fwd(d["Whh"], d["bhh"], T, Bp, P=d["P"], ids=d["ids"], h0=d["h0"], xring=4, mut=mut)
        bad = _mismatches(sr.fwd_pairs(emu, ref))
    for k in MUT_SEEN_IN[name]:
        assert k in bad, f"{name} went unnoticed in {k} (noticed in {sorted(bad)})"


def test_mismatch_flags_nan_and_reports_the_worst_element():
    ref = torch.zeros(4, 4)
    got = ref.clone()
    assert sr.mismatch(got, ref, "f32_state") is None
    got[2, 1] = float("nan")
    assert "(2, 1)" in sr.mismatch(got, ref, "f32_state")
    got[2, 1] = 1.0
    assert "(2, 1)" in sr.mismatch(got, ref, "bf16_grad")

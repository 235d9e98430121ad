"""CPU tests of models/head_ref.py: the float64 head equals autograd, the recorded emulator
deviations reproduce, every layout decoder inverts its encoder and matches the kernels' address
formulas, and every planted bug (head_ref.MUTATIONS) fails at the tolerances tests/test_head_gpu.py uses."""
import pytest
import torch

from gru_mpi_cuda_amd.models import head_ref as hr


# ------------------------------------------------------------------------------ head_ref = autograd
@pytest.mark.parametrize("kind", ["planted", "random"])
def test_head_ref_equals_autograd(kind):
    """dl, dy, dW, db and the loss of head_ref against torch.autograd of cross_entropy(sum) * inv in
    float64, 1e-10 relative to the largest entry."""
    V, H, T, Bp = 64, 48, 3, 64
    M = T * Bp
    d = hr.inputs(kind, V, H, M=M, seed=5)
    inv = float(d["inv"])
    f = torch.float64
    X = d["X"].to(f).requires_grad_()
    W = d["W"].to(f).requires_grad_()
    b = d["b"].to(f).requires_grad_()
    lg = X @ W.T + b
    lg.retain_grad()
    y = d["labels"].long()
    loss = torch.nn.functional.cross_entropy(lg, y, ignore_index=-1, reduction="sum") * inv
    loss.backward()
    ref = hr.head_ref(d["X"], d["W"], d["b"], d["labels"], inv, T=T, Bp=Bp)

    def same(a, g, what):
        assert float((a - g).abs().max()) <= 1e-10 * max(float(g.abs().max()), 1.0), what

    same(ref["loss_part"].sum(), loss.detach(), "loss")
    same(ref["nll"].sum(), loss.detach(), "nll")
    same(ref["dl"], lg.grad, "dl")
    same(ref["dy"], X.grad, "dy")
    same(ref["dW"].sum(0), W.grad, "dW")
    same(ref["db"].sum(0), b.grad, "db")
    same(ref["probs"], torch.softmax(lg.detach(), -1), "probs")
    # per row block: the reference restricted to that block's rows
    rows = torch.arange(M).reshape(T, Bp // 32, 32)
    for rb in range(Bp // 32):
        r = rows[:, rb].reshape(-1)
        same(ref["dW"][rb], ref["dl"][r].T @ d["X"].to(f)[r], f"dW[{rb}]")
        same(ref["db"][rb], ref["dl"][r].sum(0), f"db[{rb}]")


def test_softmax_xent_reference_starts_from_the_given_logits():
    d = hr.planted_inputs(128, 64)
    lg = hr.emulate(d["X"], d["W"], d["b"], d["labels"], d["inv"])["logits"]
    a = hr.head_ref(None, None, None, d["labels"], d["inv"], logits=lg)
    assert torch.equal(a["logits"], lg.double()) and "dy" not in a
    p = torch.softmax(lg.double(), -1)
    assert float((a["probs"] - p).abs().max()) < 1e-15


# ------------------------------------------------------------------------------ planted inputs
@pytest.mark.parametrize("V", [64, 128, 256, 320, 512])
def test_planted_inputs_hold_what_they_claim(V):
    H = 96
    t, y = hr.planted_table(V)
    assert torch.equal(t, t.bfloat16().float())                    # bf16-exact
    d = hr.planted_inputs(V, H)
    X, W = d["X"].double(), d["W"].double()
    assert torch.equal(X[:, :32] @ W[:, :32].T, t.double().repeat(2, 1))   # the table is added exactly
    ns, nc = V // 32, V // 64
    lab = d["labels"]
    assert bool((lab[32:] == -1).all()) and int((lab[:32] == -1).sum()) == 3   # one ignored block, scattered -1
    valid = y[y >= 0]
    assert 0 in valid and V - 1 in valid
    assert set((valid // 32).tolist()) == set(range(ns))           # a label in every 32-column slab
    assert set((t[:16].argmax(1) // 32).tolist()) == set(range(ns))   # the planted row maximum in every slab
    assert float(t[18].min()) == 100 and float(t[19].max()) == -100
    assert float(t[20, int(y[20])]) == 30 and float(t[21].max()) == 30 and float(t[21, int(y[21])]) == 0
    cm = lambda r: t[r].reshape(nc, 64).max(1).values
    if nc > 1:
        assert bool((cm(22)[1:] - cm(22)[:-1] >= 20).all()) and bool((cm(23)[1:] - cm(23)[:-1] <= -20).all())
        assert float(cm(24)[-1]) == 60 and float(cm(24)[:-1].max()) == 0
        assert sorted(cm(25).tolist())[:2] == [-100.0, 0.0]
    lg = hr.head_ref(d["X"], d["W"], d["b"], lab, d["inv"])["logits"]
    assert float(lg[18].min()) > 89, "exp(x) overflows fp32 on row 18 without the max subtraction"


# ------------------------------------------------------------------------------ layouts
def test_dlf_layout_matches_the_kernel_store():
    """Element by element against the address the FC consumer stores to (gru_seq.hip, the dlF store):
    wave column tile, row tile r, lane (lq, lr), register i -> row 16 r + 4 lq + i, the slot of lane
    (2 r + lq / 2) * 16 + lr at element (lq & 1) * 4 + i."""
    T, Bp, V = 2, 64, 48
    dl = torch.arange(T * Bp * V, dtype=torch.float32).reshape(T, Bp, V)
    F = hr.dlf_encode(dl)
    nrb = Bp // 32
    for t, rb, vt, r, lq, lr, i in [(0, 0, 0, 0, 0, 0, 0), (1, 1, 2, 1, 3, 15, 3), (0, 1, 1, 0, 2, 7, 1), (1, 0, 2, 1, 1, 9, 2)]:
        off = (((t * nrb + rb) * (V // 16) + vt) * 64 + (2 * r + (lq >> 1)) * 16 + lr) * 8 + (lq & 1) * 4 + i
        assert F[off] == dl[t, rb * 32 + r * 16 + lq * 4 + i, vt * 16 + lr]
    # the documented lane view: lane L holds rows 8 (L >> 4) .. +8 of vocab column L & 15
    blk = F.reshape(T, nrb, V // 16, 64, 8)
    assert torch.equal(blk[1, 1, 2, 37], dl[1, 32 + 16:32 + 24, 2 * 16 + 5])
    assert torch.equal(hr.dlf_decode(F, T, Bp, V), dl)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T * Bp * V, generator=g)
    assert torch.equal(hr.dlf_encode(hr.dlf_decode(x, T, Bp, V)), x)


def test_dlt_window_round_trip():
    M, V, ldT, colT = 64, 128, 80, 8
    dl = torch.arange(M * V, dtype=torch.float32).reshape(M, V)
    B = hr.dlt_encode(dl, ldT, colT, fill=-7.0)
    assert B.shape == (V, ldT) and B[5, colT + 9] == dl[9, 5]
    assert bool((B[:, :colT] == -7).all()) and bool((B[:, colT + M:] == -7).all())
    assert torch.equal(hr.dlt_decode(B, M, colT), dl)
    assert torch.equal(hr.dlt_encode(hr.dlt_decode(B, M, colT), ldT, colT, fill=-7.0), B)


# ------------------------------------------------------------------------------ tolerances
def test_tolerances_derive_from_measurement():
    for fam, dev in hr.MEASURED_DEV.items():
        assert dev > 0
        assert hr.ATOL[fam] == (max(4.0 * dev, 2.0 ** -20) if fam == "dl" else 4.0 * dev)
    assert hr.RTOL["dl"] == 2.0 ** -7 and all(v == 0 for k, v in hr.RTOL.items() if k != "dl")


def test_recorded_deviations_cover_a_fresh_measurement():
    """Re-measure |emulate - ref| (every shape is quick; two seeds): nothing exceeds the recorded
    maxima, and the recorded maxima are of the same order (not padded by hand)."""
    got = hr.measure_deviations(seeds=(0, 2))
    print({k: f"{v:.3e}" for k, v in got.items()}, hr.MEASURED_DEV)
    for fam, rec in hr.MEASURED_DEV.items():
        assert rec / 8 <= got[fam] <= rec, (fam, got[fam])


def _failures(d, form, mut=None, logits_only=False):
    """Families that miss their tolerance for one input set, with the checks of tests/test_head_gpu.py."""
    inv = float(d["inv"])
    lg = hr.emulate(d["X"], d["W"], d["b"], d["labels"], inv)["logits"] if logits_only else None
    W = None if logits_only else d["W"]
    ref = hr.head_ref(d["X"], W, d["b"], d["labels"], inv, logits=lg)
    emu = hr.emulate(d["X"], W, d["b"], d["labels"], inv, form=form, mut=mut, logits=lg)
    bad = {}
    c0 = d["dy_from"]
    checks = [("dl", emu["dl"], ref["dl"], "dl", inv), ("dlT", emu["dlT"], ref["dl"], "dl", inv),
              ("loss", emu["loss_part"], ref["loss_part"], "loss", inv), ("probs", emu["probs"], ref["probs"], "probs", 1.0)]
    if "dy" in emu:
        checks.append(("dy", emu["dy"][:, c0:], ref["dy"][:, c0:], "dy_flash" if form == "flash" else "dy", inv))
    for name, g, r, fam, n in checks:
        m = hr.mismatch(g, r, fam, n)
        if m:
            bad[name] = m
    if "dy" in emu and form == "dl":
        m = hr.gemm_mismatch(emu["dy"], emu["dl"], d["W"], d["W"].shape[0])
        if m:
            bad["dy_gemm"] = m
    ign = d["labels"] < 0
    if bool((emu["dl"][ign] != 0).any()) or ("dy" in emu and bool((emu["dy"][ign] != 0).any())):
        bad["ignored rows"] = "not exactly zero"
    if not torch.equal(emu["dlT"], emu["dl"]):
        bad["dlT == dl"] = "bits differ"
    return bad


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("V,H,form", [(64, 32, "dl"), (128, 96, "dl"), (256, 320, "dl"), (512, 128, "dl"), (256, 512, "flash")])
def test_correct_emulation_passes(V, H, form, kind):
    assert _failures(hr.inputs(kind, V, H, seed=3), form) == {}
    if form == "dl":
        assert _failures(hr.inputs(kind, V, hr.SOFTMAX_H, seed=3), form, logits_only=True) == {}


# which check must notice each planted bug
EXPECT = {
    "no_max_subtraction": "dl", "slab_missing_from_row_sum": "dl", "max_over_own_slab_only": "dl",
    "onehot_at_y_plus_1": "dl", "ignored_rows_not_zeroed": "ignored rows", "inv_applied_twice": "dl",
    "dlT_row_pairs_swapped": "dlT", "dy_last_k_step_dropped": "dy_gemm", "flash_alpha_not_applied_to_U": "dy",
    "flash_label_row_not_scaled": "dy", "uniform_softmax": "dl", "dl_zero_below_1e-4": "dl",
}


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("name", sorted(hr.MUTATIONS))
def test_planted_bug_fails_the_tolerances(name, kind):
    """Each bug on the planted and on the random inputs (V = 256, M = 64; H = 512 for the flash form).
    no_max_subtraction shows only where exp overflows: on the planted rows."""
    form = hr.MUTATIONS[name]
    d = hr.inputs(kind, 256, 512 if form == "flash" else 128, seed=3)
    bad = _failures(d, form, name)
    print(name, kind, bad)
    if name == "no_max_subtraction" and kind == "random":
        return   # logits of a few units: exp does not overflow and the result is the same softmax
    assert EXPECT[name] in bad, (name, bad)
    if name == "dy_last_k_step_dropped":
        assert "dy" in bad      # and end to end
    if name == "dlT_row_pairs_swapped":
        assert "dlT == dl" in bad


def test_the_present_tolerance_passes_a_uniform_softmax_and_small_entries_zeroed():
    """test_fc_xent (tests/test_kernels_gpu.py) compares dl with atol = 1e-4, rtol = 1e-2 at M = 128,
    V = 256.  At that tolerance the last two planted bugs pass for nearly every entry -- a uniform
    softmax for more than 95 % of dl (nine label entries in ten among them), dl = 0 below 1e-4 for all of it --
    and both fail here."""
    g = torch.Generator().manual_seed(0)
    M, V, H = 128, 256, 256
    bf = lambda t: t.bfloat16().float()
    X, W, b = bf(torch.randn(M, H, generator=g)), bf(torch.randn(V, H, generator=g) * H ** -0.5), torch.randn(V, generator=g) * 0.5
    y = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    y[::7] = -1
    inv = 1.0 / int((y >= 0).sum())
    ref = hr.head_ref(X, W, b, y, inv)["dl"]
    old_ok = lambda got: (got.double() - ref).abs() <= 1e-4 + 1e-2 * ref.abs()
    uni = hr.emulate(X, W, b, y, inv, mut="uniform_softmax")["dl"]
    small = hr.emulate(X, W, b, y, inv, mut="dl_zero_below_1e-4")["dl"]
    lab = torch.zeros(M, V, dtype=torch.bool)
    lab[y >= 0, y[y >= 0].long()] = True
    assert float(old_ok(uni).double().mean()) > 0.95 and float(old_ok(uni)[lab].double().mean()) > 0.9
    assert bool(old_ok(small).all())
    assert float(old_ok(torch.zeros(M, V)).double().mean()) > 0.9
    for got in (uni, small):
        assert hr.mismatch(got, ref, "dl", inv) is not None


def test_mismatch_flags_nan_and_reports_the_worst_element():
    ref = torch.zeros(4, 4)
    got = ref.clone()
    assert hr.mismatch(got, ref, "dl") is None
    got[2, 1] = float("nan")
    assert "(2, 1)" in hr.mismatch(got, ref, "dl")
    got[2, 1] = 1.0
    assert "(2, 1)" in hr.mismatch(got, ref, "dl") and hr.err_over_tol(got, ref, "dl") > 1
    A, B = torch.ones(2, 4), torch.ones(4, 3)
    assert hr.gemm_mismatch(A @ B, A, B, 4) is None and hr.gemm_mismatch(A @ B + 1e-4, A, B, 4) is not None
    assert hr.gemm_mismatch(torch.full((2, 3), 1e-30), torch.zeros(2, 4), B, 4) is not None   # bound 0: exactly 0


def test_clear_uniforms_moves_off_the_edges():
    import numpy as np
    p = np.array([[0.25, 0.25, 0.5], [0.1, 0.2, 0.7]])
    r, idx = hr.clear_uniforms(p, np.array([0.25, 0.05], np.float32))
    assert abs(float(r[0]) - 0.25) >= 1e-5 and float(r[1]) == np.float32(0.05)
    assert idx.tolist() == [int(np.searchsorted(np.cumsum(p[0]), float(r[0]), side="right")), 0]
    r, idx = hr.clear_uniforms(p, np.array([1.5, 0.999], np.float32))
    assert idx.tolist() == [2, 2]

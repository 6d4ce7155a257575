"""The head references (tests/head_ref.py) on the CPU: the closed-form backward against float64
autograd through the module's own forward, the loss against ops.losses.total_loss, the
rows / head_wsum_grad references against the direct gradient, the guard, and the input
conditions of every case tests/test_gpu_head_exact.py launches."""

import pytest
import torch

import exact_ref as X
import head_ref as R


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("loss,gscale", [("dice", 1.0), ("dice_bce", 1.0), ("dice_bce", 1024.0)])
def test_closed_form_backward_equals_autograd(K, loss, gscale):
    g = torch.Generator().manual_seed(10 + K)
    P, Cc = 257, 16
    x = torch.relu(torch.randn(P, Cc, generator=g, dtype=torch.float64))
    W = (torch.randn(Cc, K, generator=g, dtype=torch.float64) * 0.4).requires_grad_(True)
    b = torch.randn(K, generator=g, dtype=torch.float64).requires_grad_(True)
    t = (torch.rand(P, K, generator=g, dtype=torch.float64) > 0.6).double()
    bce_w = 0.5 if loss == "dice_bce" else 0.0
    xr = x.clone().requires_grad_(True)
    z, p, sums = R.head_forward(xr, W, b, t)
    gz, gx, gw, gb = torch.autograd.grad(gscale * R.loss_of(sums, bce_w, P * K), [z, xr, W, b])
    dz, dx, rw, rb = R.head_backward(x, W.detach(), p.detach(), t, sums.detach(), 1.0 / (P * K), bce_w, gscale)
    for name, got, want in (("dlogit", dz, gz), ("dx", dx, gx * (x > 0)), ("gw", rw, gw), ("gb", rb, gb)):
        err = ((got - want).abs().max() / want.abs().max()).item()
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("loss", ["dice", "dice_bce"])
def test_loss_equals_the_projects_loss(K, loss):
    from unet_distributed_amd.ops.losses import total_loss
    g = torch.Generator().manual_seed(20 + K)
    z32 = torch.randn(513, K, generator=g) * 3
    t = (torch.rand(513, K, generator=g) > 0.6).float()
    want, p32 = total_loss(t, z32, loss, 0.5)
    sums = R.loss_sums(z32.double(), t.double())
    got = R.loss_of(sums, 0.5 if loss == "dice_bce" else 0.0, z32.numel())
    assert abs(got.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item()))
    assert (R.sigmoid64(z32) - p32.double()).abs().max() < 1e-6


def test_rows_and_wsum_grad_reproduce_the_direct_gradient():
    """The per-workgroup rows, summed and combined by wsum_grad, are the Mask gradient of
    head_backward for every window order; each window lands in exactly one row."""
    g = torch.Generator().manual_seed(31)
    M = 7 * 512
    y = torch.relu(torch.randn(M, 32, generator=g, dtype=torch.float64))
    hw = torch.randn(32, 1, generator=g, dtype=torch.float64) * 0.2
    t = (torch.rand(M, generator=g) > 0.6).double()
    z, p, sums = R.head_forward(y, hw, torch.tensor([0.1], dtype=torch.float64), t[:, None])
    _, _, gw, gb = R.head_backward(y, hw, p, t[:, None], sums, 1.0 / M, 0.5, 8.0)
    for win_pf, rev in ((1, 0), (3, 0), (3, 1), (5, 1), (9, 0)):
        order = R.window_order(7, win_pf, rev)
        assert sorted(w for ws in order for w in ws) == list(range(7))
        assert len(order) == (7 + win_pf - 1) // win_pf and all(len(ws) == win_pf for ws in order[:-1])
        if rev:
            assert order[0][0] == 6
        rows = R.ws_rows(y, p[:, 0], t, win_pf, rev)
        assert rows.shape == (len(order), 100) and (rows[:, 99] == 0).all()
        rw, rb = R.wsum_grad(rows, sums, 1.0 / M, 0.5, 8.0)
        assert ((rw - gw[:, 0]).abs().max() / gw.abs().max()).item() < 1e-12
        assert abs((rb - gb).item()) < 1e-12 * gb.abs().item() + 1e-15
    for nwin in (1, 7, 8, 12, 37):
        o = R.window_order_cp(nwin)
        assert sorted(w for ws in o for w in ws) == list(range(nwin)) and all(len(ws) == 1 for ws in o)
        assert [ws[0] for ws in R.window_order_cp(nwin, 1)] == [nwin - 1 - ws[0] for ws in o]
    assert [ws[0] for ws in R.window_order_cp(12)] == [0, 2, 4, 6, 8, 9, 10, 11, 1, 3, 5, 7]
    rows = R.ws_rows(y, p[:, 0], t, 1, 0, order=R.window_order_cp(7))
    assert torch.allclose(R.wsum_grad(rows, sums, 1.0 / M, 0.5, 8.0)[0], gw[:, 0], rtol=1e-12, atol=0)
    # a ragged last workgroup owns the remainder; under rev it is the first windows of the tensor
    rows = R.ws_rows(y, p[:, 0], t, 5, 1)
    u, v, w = R.uvw(p[:1024, 0], t[:1024])
    assert torch.allclose(rows[1, 96:99], torch.stack([u.sum(), v.sum(), w.sum()]), rtol=1e-13, atol=0)


def test_guard_rejects_cases_outside_the_exact_regime():
    assert R.require_exact_dyadic(torch.tensor([2.0 ** 13 - 1]), 11) == 2.0 ** 13 - 1
    with pytest.raises(AssertionError, match="exact regime"):
        R.require_exact_dyadic(torch.tensor([2.0 ** 13]), 11)
    with pytest.raises(AssertionError, match="power of two"):
        R.dlogit_frac_bits(4, 1.0 / 1001, 0.5, 1.0)
    assert R.dlogit_frac_bits(4, 2.0 ** -6, 0.0, 1.0) == 10 and R.dlogit_frac_bits(4, 2.0 ** -6, 0.5, 4.0) == 9
    assert R.dlogit_frac_bits(2, 2.0 ** -10, 0.5, 1.0) == 13
    s = R.dyadic_sums()
    a, bb = R.dice_scalars(s)
    assert a == -0.5 and bb == 0.25
    p = R.dyadic_prob(3, (4000,), 4)
    assert p.min() == 1 / 16 and p.max() == 15 / 16 and R.on_grid(p, 4) and not R.on_grid(p, 3)


_DYADIC = R.dyadic_cases()


@pytest.mark.parametrize("name,make,rounded", _DYADIC, ids=[n for n, _, _ in _DYADIC])
def test_input_conditions_of_dyadic_cases(name, make, rounded):
    """Exact regime; operands representable in the storage type; every term on the 2^-frac_bits
    grid; every 16-bit output with >= 5 % of its non-zero elements needing rounding; dlogit of
    both signs."""
    case = make()
    R.require_exact_dyadic(case.bound, case.frac_bits)
    o = case.ops
    for k in ("x", "act", "wt"):
        if k in o:
            X.to_storage(o[k], case.dtype, "cpu")
    X.to_storage(o["t"], case.dtype, "cpu")
    X.to_storage(o["t"], "bf16", "cpu")
    for k in ("p", "sums", "W", "w"):
        if k in o:
            X.to_storage(o[k], "fp32", "cpu")
    dz = case.ref["dz"]
    assert R.on_grid(dz, case.frac_bits) and not R.on_grid(dz, case.frac_bits - 1), name
    assert (dz > 0).double().mean() > 0.1 and (dz < 0).double().mean() > 0.1, name
    for k, r in case.ref.items():
        assert R.on_grid(r, case.frac_bits), (name, k)
        assert torch.equal(r.float().double(), r), (name, k)
    for k in rounded:
        r = case.ref[k]
        if case.dtype == "fp16":
            assert r.abs().max() < X.FP16_MAX and r[r != 0].abs().min() >= 2.0 ** -14       # normal range
        nr, tie = X.rounding_share(r, case.dtype)
        print("%s %s: bound %.4g x 2^%d, needs rounding %.1f %%, ties %.1f %%" % (name, k, case.bound, case.frac_bits,
                                                                              100 * nr, 100 * tie))
        assert nr >= 0.05, (name, k, nr)


def test_fp16_build_cases_are_representable_in_fp16():
    assert R.FP16_BUILD
    for (P, Cc, bw, gs, dev, dt) in R.FP16_BUILD:
        case = R.bwd_case(P, Cc, 1, bw, gs, R.INV_TOTAL, dt)
        for k in ("x", "t"):
            X.to_storage(case.ops[k], "fp16", "cpu")


@pytest.mark.parametrize("nrows", R.WSUM_GRAD_ROWS)
def test_input_conditions_of_wsum_grad_rows(nrows):
    case = R.wsum_grad_case(nrows)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    for r in case.ref.values():
        assert R.on_grid(r, case.frac_bits) and torch.equal(r.float().double(), r)
    X.to_storage(case.ops["rows"], "fp32", "cpu")
    assert case.ref["gw"].abs().min() > 0 or nrows > 1


_FUSED = [(k, 0) for k in R.FUSED_HALF] + [(k[:4], k[4]) for k in R.FUSED_REAL + [R.CHAIN]]


@pytest.mark.parametrize("key,wmax", _FUSED, ids=["%s-%d" % ("x".join(map(str, k)), w) for k, w in _FUSED])
def test_input_conditions_of_fused_forward_cases(key, wmax):
    """The conv and the logit stay exact (|y| <= 64 stored without rounding, weights on the 1/64
    grid); at logit 0 every row is exact; with real weights the logits spread over about +-6
    and stay inside |z| <= 8."""
    case = R.fused_case(*key, wmax)
    conv = case.ops["conv"]
    X.require_exact(conv.bound)
    y = case.ref["y"]
    assert y.abs().max() <= 64 and y.min() >= 0
    X.to_storage(y, "bf16", "cpu")
    R.require_exact_dyadic(case.bound, case.frac_bits)
    z = case.ref["z"]
    assert torch.equal(z.float().double(), z)
    N, H, win_pf, rev = key
    grid = (N * H // 4 + win_pf - 1) // win_pf
    assert case.ref["rows"].shape == (grid, 100) and (N * H // 4) % win_pf != 0       # ragged last workgroup
    if wmax == 0:
        assert (z == 0).all() and (case.ref["p"] == 0.5).all()
        assert R.on_grid(case.ref["rows"], 2) and torch.equal(case.ref["rows"].float().double(), case.ref["rows"])
        assert case.ref["rows"][:, :96].abs().min(0).values.max() > 0
    else:
        print("fused %s: logits min %.2f max %.2f std %.2f" % (key, z.min(), z.max(), z.std()))
        assert z.abs().max() <= 8 and z.max() >= 3 and z.min() <= -3 and z.std() > 1


def test_input_conditions_of_the_3d_case():
    case = R.fused3d_case(*R.FUSED_3D)
    X.require_exact(case.ops["conv"].bound)
    y, z = case.ref["y"], case.ref["z"]
    X.to_storage(y, "bf16", "cpu")                 # 27 taps: integers up to 72, still stored without rounding
    R.require_exact_dyadic(case.bound, case.frac_bits)
    assert torch.equal(z.float().double(), z) and z.abs().max() <= 8 and z.std() > 1
    N, D, H, _ = R.FUSED_3D
    assert case.ref["rows"].shape == (N * D * H // 4, 100)
    R.require_exact_dyadic(case.dy_bound, case.dy_frac_bits)
    assert R.on_grid(case.ref["dx"], case.dy_frac_bits) and X.rounding_share(case.ref["dx"], "bf16")[0] >= 0.05


@pytest.mark.parametrize("key", R.HEAD_FWD, ids=["x".join(map(str, k)) for k in R.HEAD_FWD])
def test_input_conditions_of_head_fwd_cases(key):
    case = R.fwd_case(*key)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    z = case.ref["z"]
    X.to_storage(case.ops["x"], "bf16", "cpu")
    assert R.on_grid(z, 6) and torch.equal(z.float().double(), z)
    print("head_fwd %s: logits min %.2f max %.2f std %.2f" % (key, z.min(), z.max(), z.std()))
    assert z.abs().max() <= 8 and z.max() >= 4 and z.min() <= -4 and z.std() > 1.5


def test_input_conditions_of_head_finish_cases():
    for P in R.FINISH:
        z = R.finish_case(P).ops["z"]
        assert R.on_grid(z, 6) and z.abs().max() <= 6 and z.std() > 3
    for P in R.FINISH_HALF:
        c = R.finish_half_case(P)
        s = c.ref["sums"]
        assert R.on_grid(s[:3], 1) and torch.equal(s[:3].float().double(), s[:3]) and s[2] == P / 2
    c = R.finish_half_case(1001, False)
    assert c.ref["sums"].tolist() == [0.0, 0.0, 500.5, 0.0]
    # more than one grid-stride round needs more than 4096 blocks x 256 threads x 4 pixels
    assert R.FINISH_HALF[-1] // 4 > 4096 * 256 and R.FINISH_HALF[-1] % 4 == 3


_TARGETS = R.target_cases()


@pytest.mark.parametrize("name,make", _TARGETS, ids=[n for n, _ in _TARGETS])
def test_targets_are_on_between_10_and_90_percent_of_pixels(name, make):
    t = make()
    share = t.double().mean().item()
    assert set(t.unique().tolist()) <= {0.0, 1.0} and 0.1 <= share <= 0.9, (name, share)

"""The segmentation head and loss kernels against float64 CPU references (tests/head_ref.py).

Bit for bit wherever the arithmetic allows it: the backward kernels (head_bwd, head_mc_bwd,
head_dy, the head-on-load data / weight gradients, head_wsum_grad) take the probabilities,
targets, sums and scalars as plain inputs, and dyadic values keep every fp32 value exact; at
logit 0 the sigmoid is exactly 1/2, so the fused-head forward's rows and head_finish's counts
are exact too.  The sigmoid, the BCE and the rows with real head weights are held to named
bounds: 4 x the worst error measured on an MI355X (profiles/r22_head_exact.md), never above
1e-5 absolute on a probability and 1e-5 sum |terms| on a sum, a row or a gradient.

Each case prints one `HEAD|case|kernel|max abs err|bound|ms` line."""

import time

import pytest
import torch

import exact_ref as X
import head_ref as R
from test_gpu_exact import DT, S, f32, fwd_dict, fwd_ptrs, geo, nan16, pack_wd, run_wgrad
from test_gpu_kernels import C, ptr, stream
from test_gpu_multiclass import Guarded

pytestmark = pytest.mark.gpu

# Ceilings (fp32 evaluation at |z| <= 8 with <= 2^16 terms stays near 1e-6; one pixel with the
# wrong target out of 49 152 is above 1e-4).  No bound below may exceed them.
CEIL_PROB = 1e-5
CEIL_REL = 1e-5
# 4 x the worst error measured on an MI355X, relative to sum |terms| unless absolute
# (profiles/r22_head_exact.md).  The margin of 4 covers another reduction grouping when
# head_blocks or win_pf change and the growth of __expf's error with |z|.
PROB_ABS = 3.2e-7                   # measured 7.76e-8 (head_finish, P = 4096)
SUM_I_REL = 2.8e-7                  # measured 7.00e-8 (head_finish after the fused forward, 49 152 pixels)
SUM_SP_REL = 2.8e-7                 # measured 6.85e-8 (head_finish, P = 1001)
SUM_BCE_REL = 8.9e-7                # measured 2.22e-7 (head_finish at logit 0, P = 4 195 331)
ROW_REL = 7.0e-7                    # measured 1.73e-7 (3D rows; 2D: 1.60e-7)
ROW_TOTAL_REL = 3.4e-7              # measured 8.47e-8 (3 x 8 x 128, win_pf = 5, rev = 1)
CHAIN_GRAD_REL = 5.7e-7             # measured 1.42e-7: fused forward -> head_finish -> head_wsum_grad
WSUM_GRAD_REL = 4.2e-7              # measured 1.04e-7: head_wsum_grad on the reference's rows and sums
for _b in (SUM_I_REL, SUM_SP_REL, SUM_BCE_REL, ROW_REL, ROW_TOTAL_REL, CHAIN_GRAD_REL, WSUM_GRAD_REL):
    assert _b <= CEIL_REL
assert PROB_ABS <= CEIL_PROB
NAN = float("nan")


def line(case, kernel, err, bound, t0):
    print("HEAD|%s|%s|%.3g|%.3g|%.0f" % (case, kernel, err, bound, 1e3 * (time.perf_counter() - t0)))


def nan32(n):
    return torch.full((int(n),), NAN, device="cuda")


def bits_eq(out, ref64, what, dtype="fp32"):
    X.assert_bits_equal(out.reshape(ref64.shape), X.rne(ref64, dtype), what, ref64, dtype)


def maxerr(out, ref64):
    return (out.detach().cpu().double().reshape(ref64.shape) - ref64).abs().max().item()


def scale_args(gs, dev):
    """-> (floats' loss scale, extra pointer list, keep-alive): through the device pointer the
    float argument is 1 and must be ignored."""
    if not dev:
        return gs, [], None
    sc = f32(torch.tensor([gs], dtype=torch.float64))
    return 1.0, [ptr(sc)], sc


# ----------------------------------------------------------------- dyadic: head_bwd
def run_head_bwd(case, K, dev, dtype, want_dx=True):
    o = case.ops
    P, Cc = o["x"].shape
    x, t = S(o["x"], dtype), S(o["t"].reshape(-1), dtype)
    w, prob, sums = f32(o["W"].reshape(-1)), f32(o["p"].reshape(-1)), f32(o["sums"])
    inv_total, bce_w, gs = case.scal
    part = nan32(C().head_blocks(P) * (Cc + 1) * K)
    dx = nan16((P, Cc), dtype)
    gw, gb = Guarded(Cc * K, torch.float32, "cuda"), Guarded(K, torch.float32, "cuda")
    gsf, extra, keep = scale_args(gs, dev)
    C().generic("head_bwd", [ptr(x), ptr(w), ptr(prob), ptr(t), ptr(sums), ptr(dx) if want_dx else 0, ptr(part),
                             ptr(gw.out), ptr(gb.out)] + extra, [P, Cc] + ([K] if K > 1 else []),
                [inv_total, bce_w, gsf], stream(), dtype=DT[dtype])
    torch.cuda.synchronize()
    gw.check()
    gb.check()
    return dx, gw.out, gb.out


def check_head_bwd(name, case, K, dev, dtype, t0):
    R.require_exact_dyadic(case.bound, case.frac_bits)
    dx, gw, gb = run_head_bwd(case, K, dev, dtype)
    r = case.ref
    line(name, "head_bwd" if K == 1 else "head_mc_bwd", max(maxerr(dx, X.rne(r["dx"], dtype).double()),
                                                            maxerr(gw, r["gw"]), maxerr(gb, r["gb"])), 0, t0)
    X.assert_bits_equal(dx, X.rne(r["dx"], dtype), "%s dx" % name, r["dx"], dtype)
    bits_eq(gw, r["gw"], "%s gw" % name)
    bits_eq(gb, r["gb"], "%s gb" % name)
    return dx, gw, gb


@pytest.mark.parametrize("key", R.BWD_K1, ids=["x".join(map(str, k)) for k in R.BWD_K1])
def test_head_bwd_single_class(cuda_dev, key):
    """dx, gw, gb of head_bwd (16 / 32 / 64 channels, an odd pixel count and more than one
    round, Dice and Dice + BCE, the loss scale as argument and through the device pointer, the
    fp16 build), and with dx = nullptr the same gw / gb."""
    t0 = time.perf_counter()
    P, Cc, bw, gs, dev, dtype = key
    case = R.bwd_case(P, Cc, 1, bw, gs, R.INV_TOTAL, dtype)
    name = "bwd %s" % (key,)
    check_head_bwd(name, case, 1, dev, dtype, t0)
    dx, gw, gb = run_head_bwd(case, 1, dev, dtype, want_dx=False)
    assert torch.isnan(dx.float()).all(), "dx == nullptr: nothing is written"
    bits_eq(gw, case.ref["gw"], "%s gw without dx" % name)
    bits_eq(gb, case.ref["gb"], "%s gb without dx" % name)


@pytest.mark.parametrize("key", R.BWD_MC, ids=["x".join(map(str, k)) for k in R.BWD_MC])
def test_head_bwd_multi_class(cuda_dev, key):
    t0 = time.perf_counter()
    P, Cc, K, bw, gs, dev = key
    case = R.bwd_case(P, Cc, K, bw, gs, R.INV_TOTAL)
    check_head_bwd("bwd mc %s" % (key,), case, K, dev, "bf16", t0)


def run_head_dy(bits, w64, p64, t64, sums64, scal, dev, P, Cc):
    w, prob, t, sums = f32(w64.reshape(-1)), f32(p64.reshape(-1)), S(t64.reshape(-1)), f32(sums64)
    inv_total, bce_w, gs = scal
    dx = nan16((P, Cc))
    gsf, extra, keep = scale_args(gs, dev)
    C().generic("head_dy", [ptr(bits), ptr(w), ptr(prob), ptr(t), ptr(sums), ptr(dx)] + extra, [P, Cc],
                [inv_total, bce_w, gsf], stream())
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("key", R.HEAD_DY, ids=["x".join(map(str, k)) for k in R.HEAD_DY])
def test_head_dy_from_relu_bits(cuda_dev, key):
    """head_dy forms head_bwd's dx from the packed ReLU bits: the head_bwd reference of the
    same operands."""
    t0 = time.perf_counter()
    P, Cc, bw, gs, dev = key
    case = R.bwd_case(P, Cc, 1, bw, gs, R.INV_TOTAL)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    o = case.ops
    bits = X.pack_bits(o["x"]).cuda()
    dx = run_head_dy(bits, o["W"], o["p"], o["t"], o["sums"], case.scal, dev, P, Cc)
    line("dy %s" % (key,), "head_dy", maxerr(dx, X.rne(case.ref["dx"], "bf16").double()), 0, t0)
    X.assert_bits_equal(dx, X.rne(case.ref["dx"], "bf16"), "head_dy %s" % (key,), case.ref["dx"], "bf16")


# ------------------------------------------------------------ dyadic: head-on-load
ONLOAD_IDS = ["%dx%dx%dx%d%s" % (k[0], k[1], k[2], k[3], "-pf" if k[6] else "") for k in R.ONLOAD]


def onload_operands(case, gs):
    o = case.ops
    keep = dict(x=S(o["x"]), prob=f32(o["p"].reshape(-1)), t=S(o["t"].reshape(-1)), sums=f32(o["sums"]),
                w=f32(o["w"]), bits=X.pack_bits(o["x"]).cuda(), gsc=f32(torch.tensor([gs], dtype=torch.float64)))
    inv_total, bce_w, _ = case.scal
    hg = dict(hg_prob=ptr(keep["prob"]), hg_t=ptr(keep["t"]), hg_sums=ptr(keep["sums"]), hg_w=ptr(keep["w"]),
              hg_bits=ptr(keep["bits"]), hg_gscale=ptr(keep["gsc"]), hg_inv_total=inv_total, hg_bce_w=bce_w)
    return keep, hg


@pytest.mark.parametrize("key", R.ONLOAD, ids=ONLOAD_IDS)
def test_head_onload_data_gradient(cuda_dev, key):
    """XF 3: the 3x3 data gradient of the head-input conv forming dY = dlogit w (x > 0) in LDS
    from probability, target and ReLU bits (plain and persistent window):
    RNE(conv_dgrad(RNE(dY), w) (act > 0))."""
    t0 = time.perf_counter()
    N, H, Wd, Cy, bw, gs, var = key
    case = R.onload_case(N, H, Wd, Cy, bw, gs, R.INV_TOTAL)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    keep, hg = onload_operands(case, gs)
    o = case.ops
    abits, wp = X.pack_bits(o["act"]).cuda(), pack_wd(o["wt"], "bf16")
    dx = nan16(case.ref["dx"].shape)
    # (src1: dY is formed on load, the pointer only has to be valid)
    d = dict(geo(N, 1, H, Wd), C1=32, src1=ptr(keep["x"]), wgt=ptr(wp), Cout=Cy, mask1=ptr(abits), mask_bits=1,
             dst1=ptr(dx), **hg, **var)
    pick = C().conv_fwd_pick(d)
    assert pick == 6, pick
    if var:
        assert C().conv_fwd_grid(d) == (N * H // 4 + var["win_pf"] - 1) // var["win_pf"]
    C().conv_fwd(d, stream())
    torch.cuda.synchronize()
    line("onload dgrad %s" % (key[:6],), "conv_fwd pick %d %s" % (pick, var), maxerr(dx, X.rne(case.ref["dx"], "bf16").double()),
         0, t0)
    X.assert_bits_equal(dx, X.rne(case.ref["dx"], "bf16"), "head-on-load data gradient %s" % (key,), case.ref["dx"], "bf16")


@pytest.mark.parametrize("splits", R.ONLOAD_SPLITS)
@pytest.mark.parametrize("key", R.ONLOAD, ids=ONLOAD_IDS)
def test_head_onload_weight_gradient(cuda_dev, key, splits):
    """The on-load weight / bias gradient of the head-input conv: the reduced fp32 slabs equal
    conv_wgrad([act], RNE(dY))."""
    t0 = time.perf_counter()
    N, H, Wd, Cy, bw, gs, var = key
    case = R.onload_case(N, H, Wd, Cy, bw, gs, R.INV_TOTAL)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    keep, hg = onload_operands(case, gs)
    a = S(case.ops["act"])
    d = dict(N=N, QH=H, QW=Wd, AH=H, AW=Wd, KH=3, KW=3, pad=1, M1=Cy, a1=ptr(a), b=ptr(keep["x"]), Nc=32, bias_mode=1,
             **hg)
    gw, gb = run_wgrad(d, splits, 9, Cy, Cy, 32, (splits, 32))
    line("onload wgrad %s splits=%d" % (key[:6], splits), "wgrad", max(maxerr(gw, case.ref["gw"]), maxerr(gb, case.ref["gb"])),
         0, t0)
    bits_eq(gw, case.ref["gw"], "head-on-load weight gradient %s" % (key,))
    bits_eq(gb, case.ref["gb"], "head-on-load bias gradient %s" % (key,))


# ------------------------------------------------------------ dyadic: head_wsum_grad
def run_wsum_grad(rows, sums, scal, nrows):
    gw, gb = Guarded(32, torch.float32, "cuda"), Guarded(1, torch.float32, "cuda")
    C().generic("head_wsum_grad", [ptr(rows), ptr(sums), ptr(gw.out), ptr(gb.out)], [nrows], list(scal), stream())
    torch.cuda.synchronize()
    gw.check()
    gb.check()
    return gw.out, gb.out


@pytest.mark.parametrize("nrows", R.WSUM_GRAD_ROWS)
def test_head_wsum_grad_alone(cuda_dev, nrows):
    """Hand-built dyadic rows: the float64 column sums times the dyadic scalars, through the
    serial loop (<= 256 rows) and the 256-wide tree (300 rows)."""
    t0 = time.perf_counter()
    case = R.wsum_grad_case(nrows)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    rows, sums = f32(case.ops["rows"]), f32(case.ops["sums"])
    gw, gb = run_wsum_grad(rows, sums, case.scal, nrows)
    line("wsum_grad rows=%d" % nrows, "head_wsum_grad", max(maxerr(gw, case.ref["gw"]), maxerr(gb, case.ref["gb"])), 0, t0)
    bits_eq(gw, case.ref["gw"], "head_wsum_grad gw, %d rows" % nrows)
    bits_eq(gb, case.ref["gb"], "head_wsum_grad gb, %d rows" % nrows)


# ------------------------------------------------- the fused-head forward's rows
GUARD_ROWS = 8


def run_fused(case, N, D, H, var):
    """The fused-head forward with the Mask weight sums, the head input not stored.  ->
    (rows [grid, 100], logits [M], ReLU bits, grid); checks the guard rows."""
    o = case.ops
    keep = []
    P = fwd_ptrs(o["conv"], "bf16", keep)
    M = N * D * H * 128
    hw, hb, t = f32(o["hw"]), f32(o["hb"]), S(o["t"])
    logit = Guarded(M, torch.float32, "cuda")
    bits = torch.full((M * 4,), 0xA5, device="cuda", dtype=torch.uint8)
    d = dict(fwd_dict((N, D, H, 128, 32, 0, 32, 0), dict(P, y=None)), head_w=ptr(hw), head_b=ptr(hb),
             head_logit=ptr(logit.out), head_t=ptr(t), relu_bits=ptr(bits), head_nostore=1, **var)
    grid = int(C().conv_fwd_grid(dict(d, head_ws=1)))
    assert grid == case.ref["rows"].shape[0], (grid, case.ref["rows"].shape)
    ws = torch.full((grid + 2 * GUARD_ROWS, 100), NAN, device="cuda")
    d.update(head_ws=ptr(ws[GUARD_ROWS:]), head_ws_rows=grid)
    assert C().conv_fwd_pick(d) == 6
    C().conv_fwd(d, stream())
    torch.cuda.synchronize()
    logit.check()
    assert torch.isnan(ws[:GUARD_ROWS]).all() and torch.isnan(ws[GUARD_ROWS + grid:]).all(), "rows past the grid stay NaN"
    rows = ws[GUARD_ROWS:GUARD_ROWS + grid]
    assert torch.isfinite(rows).all()
    return rows, logit.out, bits, grid


@pytest.mark.parametrize("key", R.FUSED_HALF, ids=["x".join(map(str, k)) for k in R.FUSED_HALF])
def test_fused_head_rows_at_logit_zero(cuda_dev, key):
    """Head weights and bias zero: logit 0, p = 1/2 (the epilogue's rcp(1 + __expf(-0)) is
    exactly 1/2 on gfx950, profiles/r22_head_exact.md), u = t / 4, v = 1 / 4, w = 1 / 2 - t:
    every row of every workgroup (ragged last one, both walk orders) bit for bit, pad 0."""
    t0 = time.perf_counter()
    N, H, win_pf, rev = key
    case = R.fused_case(N, H, win_pf, rev, 0)
    X.require_exact(case.ops["conv"].bound)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    rows, logit, bits, grid = run_fused(case, N, 1, H, dict(win_pf=win_pf, rev=rev))
    assert grid == (N * H // 4 + win_pf - 1) // win_pf
    line("fused half %s" % (key,), "conv_fwd head_ws grid=%d" % grid, maxerr(rows, case.ref["rows"]), 0, t0)
    bits_eq(rows, case.ref["rows"], "head_ws rows at logit 0 %s" % (key,))
    assert (rows[:, 99] == 0).all(), "pad float"
    bits_eq(logit, case.ref["z"], "logit")
    X.assert_bits_equal(bits, X.pack_bits(case.ref["y"]).reshape(-1), "ReLU bits of the unstored head input")


def rows_errors(rows, case):
    ref, ab = case.ref["rows"], case.ref["rows_abs"]
    err = (rows.detach().cpu().double() - ref).abs()
    live = ab > 0
    assert (err[~live] == 0).all()
    per_row = (err[live] / ab[live]).max().item()
    tot = ab.sum(0)
    total = (rows.detach().cpu().double().sum(0) - ref.sum(0)).abs()[tot > 0] / tot[tot > 0]
    return per_row, total.max().item(), err.max().item()


@pytest.mark.parametrize("key", R.FUSED_REAL, ids=["x".join(map(str, k)) for k in R.FUSED_REAL])
def test_fused_head_rows_with_real_weights(cuda_dev, key):
    """Head weights on the 1/64 grid: the fp32 logit is still exact; the rows within ROW_REL
    of sum |terms| per entry and ROW_TOTAL_REL summed over the workgroups."""
    t0 = time.perf_counter()
    N, H, win_pf, rev, wmax = key
    case = R.fused_case(N, H, win_pf, rev, wmax)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    rows, logit, bits, grid = run_fused(case, N, 1, H, dict(win_pf=win_pf, rev=rev))
    per_row, total, mx = rows_errors(rows, case)
    line("fused real %s" % (key,), "conv_fwd head_ws rows (rel)", per_row, ROW_REL, t0)
    line("fused real %s" % (key,), "conv_fwd head_ws total (rel)", total, ROW_TOTAL_REL, t0)
    bits_eq(logit, case.ref["z"], "logit")
    X.assert_bits_equal(bits, X.pack_bits(case.ref["y"]).reshape(-1), "ReLU bits of the unstored head input")
    assert (rows[:, 99] == 0).all(), "pad float"
    assert per_row <= ROW_REL and total <= ROW_TOTAL_REL, (per_row, total)


# --------------------------------------------------------------------- head_finish
def run_finish(z64, t64):
    P = z64.numel()
    prob = Guarded(P, torch.float32, "cuda")
    prob.out.copy_(z64.float())
    assert torch.equal(prob.out.cpu().double(), z64)
    t = S(t64) if t64 is not None else None
    part = nan32(4 * 4096 + 64)
    sums = Guarded(4, torch.float32, "cuda")
    C().generic("head_finish", [ptr(prob.out), ptr(t) if t is not None else 0, ptr(part), ptr(sums.out)], [P], [], stream())
    torch.cuda.synchronize()
    prob.check()
    sums.check()
    return prob.out, sums.out


def sums_errors(sums, case):
    ref, terms = case.ref["sums"], case.ref["terms"]
    err = (sums.detach().cpu().double() - ref).abs()
    return [(err[k] / terms[k]).item() if terms[k] > 0 else err[k].item() for k in range(4)]


def check_sums(name, kernel, prob, sums, case, t0):
    """Probabilities within PROB_ABS, I / Sp / BCE within their bounds of sum |terms|, St (a
    count below 2^24) exact."""
    ep = maxerr(prob, case.ref["p"])
    eI, eT, eP, eB = sums_errors(sums, case)
    for what, e, b in (("prob (abs)", ep, PROB_ABS), ("I (rel)", eI, SUM_I_REL), ("St", eT, 0), ("Sp (rel)", eP, SUM_SP_REL),
                       ("BCE (rel)", eB, SUM_BCE_REL)):
        line(name, "%s %s" % (kernel, what), e, b, t0)
    assert ep <= PROB_ABS and eI <= SUM_I_REL and eT == 0 and eP <= SUM_SP_REL and eB <= SUM_BCE_REL, (ep, eI, eT, eP, eB)


@pytest.mark.parametrize("P", R.FINISH_HALF)
def test_head_finish_at_logit_zero(cuda_dev, P):
    """prob exactly 1/2 in the 4-pixel body and the scalar tail (P = 1, 3: tail only; the largest
    P: a second grid-stride round and a tail); I, St, Sp the float64 counts bit for bit."""
    t0 = time.perf_counter()
    case = R.finish_half_case(P)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    prob, sums = run_finish(case.ops["z"], case.ops["t"])
    eB = sums_errors(sums, case)[3]
    line("finish half P=%d" % P, "head_finish BCE (rel)", eB, SUM_BCE_REL, t0)
    assert (prob == 0.5).all(), (prob != 0.5).nonzero()[:8]
    bits_eq(sums[:3], case.ref["sums"][:3], "I, St, Sp at logit 0, P = %d" % P)
    assert eB <= SUM_BCE_REL, eB


def test_head_finish_without_target(cuda_dev):
    """t == nullptr: probabilities and Sp only; I = St = BCE = 0."""
    t0 = time.perf_counter()
    case = R.finish_half_case(1001, False)
    prob, sums = run_finish(case.ops["z"], None)
    line("finish half P=1001 no target", "head_finish", maxerr(sums, case.ref["sums"]), 0, t0)
    assert (prob == 0.5).all()
    bits_eq(sums, case.ref["sums"], "sums without a target")


@pytest.mark.parametrize("P", R.FINISH)
def test_head_finish_probabilities_and_sums(cuda_dev, P):
    t0 = time.perf_counter()
    case = R.finish_case(P)
    prob, sums = run_finish(case.ops["z"], case.ops["t"])
    check_sums("finish P=%d" % P, "head_finish", prob, sums, case, t0)


# ------------------------------------------------------------------------ head_fwd
@pytest.mark.parametrize("key", R.HEAD_FWD, ids=["x".join(map(str, k)) for k in R.HEAD_FWD])
def test_head_fwd_probabilities_and_sums(cuda_dev, key):
    """head_fwd (K = 1) and head_mc_fwd (K = 2..4): exact fp32 logits (integer activations,
    weights on the 1/64 grid), probabilities and all four sums against float64."""
    t0 = time.perf_counter()
    P, Cc, K = key
    case = R.fwd_case(P, Cc, K)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    o = case.ops
    x, w, b, t = S(o["x"]), f32(o["W"].reshape(-1)), f32(o["b"]), S(o["t"].reshape(-1))
    nb = C().head_blocks(P)
    prob, sums = Guarded(P * K, torch.float32, "cuda"), Guarded(4, torch.float32, "cuda")
    part = nan32(nb * (Cc + 1) * K + 4 * nb)
    C().generic("head_fwd", [ptr(x), ptr(w), ptr(b), ptr(t), ptr(prob.out), ptr(part), ptr(sums.out)],
                [P, Cc] + ([K] if K > 1 else []), [], stream())
    torch.cuda.synchronize()
    prob.check()
    sums.check()
    check_sums("fwd %s" % (key,), "head_fwd" if K == 1 else "head_mc_fwd", prob.out, sums.out, case, t0)


# ------------------------------------------------- the shipped Mask-gradient chain
def test_mask_gradient_chain(cuda_dev):
    """fused forward (3 x 128 x 128, win_pf = 5) -> head_finish -> head_wsum_grad, the kernels
    the default 128 x 128 step runs for the Mask gradient, against the float64 gradient of the
    loss; then head_wsum_grad alone on the reference's rows and sums (its own error, apart
    from the forward's)."""
    t0 = time.perf_counter()
    N, H, win_pf, rev, wmax = R.CHAIN
    case = R.fused_case(N, H, win_pf, rev, wmax)
    y, t, M = case.ref["y"], case.ops["t"], N * H * 128
    scal = (1.0 / M, 0.5, 1.0)
    sums64 = R.loss_sums(case.ref["z"], t)
    dz, _, gw64, gb64 = R.head_backward(y, case.ops["hw"][:, None], case.ref["p"][:, None], t[:, None], sums64, *scal)
    _, gwa, gba = R.head_grads(y, case.ops["hw"][:, None], dz.abs())               # sum |terms|
    rows, logit, bits, grid = run_fused(case, N, 1, H, dict(win_pf=win_pf, rev=rev))
    tdev = S(t)
    part, sums = nan32(4 * 4096 + 64), Guarded(4, torch.float32, "cuda")
    C().generic("head_finish", [ptr(logit), ptr(tdev), ptr(part), ptr(sums.out)], [M], [], stream())
    torch.cuda.synchronize()
    sums.check()
    fin = R.Case(ref=dict(p=case.ref["p"], sums=sums64, terms=R.sum_terms(case.ref["z"], t)))
    check_sums("chain", "head_finish", logit, sums.out, fin, t0)
    rows = rows.contiguous()
    gw, gb = run_wsum_grad(rows, sums.out, scal, grid)
    e1 = max(((gw.cpu().double() - gw64[:, 0]).abs() / gwa[:, 0]).max().item(), (abs(gb.item() - gb64.item()) / gba.item()))
    line("chain", "fwd + finish + wsum_grad gw, gb (rel)", e1, CHAIN_GRAD_REL, t0)
    gw2, gb2 = run_wsum_grad(f32(case.ref["rows"].float().double()), f32(sums64.float().double()), scal, grid)
    e2 = max(((gw2.cpu().double() - gw64[:, 0]).abs() / gwa[:, 0]).max().item(), (abs(gb2.item() - gb64.item()) / gba.item()))
    line("chain", "wsum_grad on reference rows and sums (rel)", e2, WSUM_GRAD_REL, t0)
    assert e1 <= CHAIN_GRAD_REL and e2 <= WSUM_GRAD_REL, (e1, e2)


# ------------------------------------------------------------------------------- 3D
def test_fused_head_rows_and_head_dy_3d(cuda_dev):
    """The 3D head_wsum path at kernel level: the 128-wide chunk-pipelined fused-head window
    (one 512-pixel window per workgroup) writes exact logits, ReLU bits and the rows; head_dy
    then forms the head input's dY from those bits (dyadic operands: bit for bit)."""
    t0 = time.perf_counter()
    N, D, H, wmax = R.FUSED_3D
    case = R.fused3d_case(N, D, H, wmax)
    X.require_exact(case.ops["conv"].bound)
    R.require_exact_dyadic(case.bound, case.frac_bits)
    rows, logit, bits, grid = run_fused(case, N, D, H, dict(win_cp=2))
    assert grid == N * D * H // 4
    per_row, total, mx = rows_errors(rows, case)
    line("fused 3d %s" % (R.FUSED_3D,), "conv_fwd head_ws rows (rel)", per_row, ROW_REL, t0)
    line("fused 3d %s" % (R.FUSED_3D,), "conv_fwd head_ws total (rel)", total, ROW_TOTAL_REL, t0)
    bits_eq(logit, case.ref["z"], "3D logit")
    X.assert_bits_equal(bits, X.pack_bits(case.ref["y"]).reshape(-1), "3D ReLU bits")
    assert per_row <= ROW_REL and total <= ROW_TOTAL_REL, (per_row, total)
    R.require_exact_dyadic(case.dy_bound, case.dy_frac_bits)
    o = case.ops
    M = N * D * H * 128
    dx = run_head_dy(bits, o["wi"], o["pd"], o["t"], o["sums"], case.scal, False, M, 32)
    line("fused 3d %s" % (R.FUSED_3D,), "head_dy from the forward's bits", maxerr(dx, X.rne(case.ref["dx"], "bf16").double()), 0, t0)
    X.assert_bits_equal(dx, X.rne(case.ref["dx"], "bf16"), "3D head_dy", case.ref["dx"], "bf16")

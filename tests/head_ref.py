"""Float64 references of the segmentation head and its loss, and the dyadic operands that make
most of the head's backward bit-exact (tests/test_gpu_head_exact.py, tests/test_head_ref_cpu.py).

The formulas are the ones in the headers of csrc/kernels/head.hip and head_mc.hip:

    z[p][k] = sum_c x[p][c] W[c][k] + b[k],  prob = sigmoid(z)
    I = sum t prob, St = sum t, Sp = sum prob, BCE = sum max(z, 0) - z t + log1p(exp(-|z|))
    loss = -log(2 I + 1) + log(St + Sp + 1) + bce_w BCE / (P K)
    dlogit = g ((a t + bb) prob (1 - prob) + bce_w (prob - t) inv_total),
             a = -2 / (2 I + 1), bb = 1 / (St + Sp + 1)
    dx[p][c] = (x[p][c] > 0) sum_k dlogit[p][k] W[c][k]
    gw[c][k] = sum_p dlogit[p][k] x[p][c],  gb[k] = sum_p dlogit[p][k]

everything in float64 on the CPU (ops.losses.total_loss casts to fp32 and is only tied to
this module by a CPU test).

The backward kernels take prob, t, sums, inv_total, bce_w and the loss scale as plain inputs.
With sums = {1.5, s, 3 - s, .} (a = -1/2, bb = 1/4), prob = k / 2^pbits, t in {0, 1}, powers
of two for inv_total, bce_w and the loss scale, and small integer weights and activations,
every value of head_grad.h's head_dlogit (both fused multiply-adds included) and every
product and partial sum behind it is a multiple of 2^-frac_bits below 2^(24 - frac_bits):
exact in fp32 in any order.  A stored 16-bit value must then be the round-to-nearest-even
image of the float64 result and an fp32 gradient must equal it.

Plain helper module, imported like exact_ref: references, operand generators, the guard and
the case tables (so that the CPU test checks every case's conditions without a GPU).
"""

import functools
import math

import torch

import exact_ref as X

Case = X.Case


# --------------------------------------------------------------------------- references
def sigmoid64(z):
    return torch.sigmoid(z.double())


def bce_terms(z, t):
    z, t = z.double(), t.double()
    return z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))


def loss_sums(z, t=None):
    """{I, St, Sp, BCE} of logits z and targets t (same shape); t None: Sp only."""
    p = sigmoid64(z)
    if t is None:
        return torch.stack([torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), p.sum(),
                            torch.zeros((), dtype=torch.float64)])
    t = t.double()
    return torch.stack([(t * p).sum(), t.sum(), p.sum(), bce_terms(z, t).sum()])


def sum_terms(z, t=None):
    """sum |terms| of each of the four sums (the scale of their error bounds)."""
    p = sigmoid64(z)
    if t is None:
        return torch.stack([p.sum() * 0, p.sum() * 0, p.sum(), p.sum() * 0])
    t = t.double()
    return torch.stack([(t * p).sum(), t.sum(), p.sum(), bce_terms(z, t).abs().sum()])


def head_forward(x, W, b, t=None):
    """x [P, C], W [C, K], b [K], t [P, K] -> logits [P, K], probabilities, sums[4]"""
    z = x.double() @ W.double() + b.double()
    return z, sigmoid64(z), loss_sums(z, t)


def loss_of(sums, bce_w, total):
    """The training loss from the four sums (`total` = P K elements)."""
    return -torch.log(2 * sums[0] + 1) + torch.log(sums[1] + sums[2] + 1) + bce_w * sums[3] / total


def dice_scalars(sums):
    return -2.0 / (2.0 * sums[0] + 1.0), 1.0 / (sums[1] + sums[2] + 1.0)


def dlogit(p, t, sums, inv_total, bce_w, gscale):
    """Closed-form gradient of gscale * loss with respect to the logits."""
    p, t = p.double(), t.double()
    a, bb = dice_scalars(sums.double())
    return gscale * ((a * t + bb) * p * (1 - p) + bce_w * (p - t) * inv_total)


def head_grads(x, W, dz):
    """dz [P, K] -> dx [P, C] (masked by x > 0), gw [C, K], gb [K]"""
    x, W, dz = x.double(), W.double(), dz.double()
    return (dz @ W.t()) * (x > 0), x.t() @ dz, dz.sum(0)


def head_backward(x, W, p, t, sums, inv_total, bce_w, gscale):
    dz = dlogit(p, t, sums, inv_total, bce_w, gscale)
    return (dz,) + head_grads(x, W, dz)


def uvw(p, t):
    """The per-pixel factors of dlogit = A u + B v + G w (conv_params.h head_ws)."""
    p, t = p.double(), t.double()
    v = p * (1 - p)
    return t * v, v, p - t


def window_order(nwin, win_pf, rev):
    """Windows (4 rows x 128 pixels of the N H rows) of each workgroup: workgroup b owns
    [b win_pf, (b + 1) win_pf) of the walk, the walk mirrored under rev."""
    grid = (nwin + win_pf - 1) // win_pf
    out = []
    for b in range(grid):
        ws = range(b * win_pf, min((b + 1) * win_pf, nwin))
        out.append([nwin - 1 - w if rev else w for w in ws])
    return out


def xcd_remap(bid, nwg):
    """common.h xcd_remap: workgroups dealt round-robin over 8 XCDs take contiguous tile ranges"""
    q, r = divmod(nwg, 8)
    xcd, idx = bid % 8, bid // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def window_order_cp(nwin, rev=0):
    """The chunk-pipelined window (3D fused head): one window per workgroup, workgroup b takes
    window xcd_remap(b), mirrored under rev; its row is row b."""
    return [[nwin - 1 - xcd_remap(b, nwin) if rev else xcd_remap(b, nwin)] for b in range(nwin)]


def ws_rows(y, p, t, win_pf, rev, absolute=False, order=None):
    """The fused-head forward's rows: y [M, 32] stored head input, p / t [M] -> [grid, 100]:
    {sum u y_c, sum v y_c, sum w y_c} (3 x 32), sum u, sum v, sum w, 0 per workgroup.
    order: the windows of each workgroup (default: the persistent window's window_order).
    absolute: sums of |terms|."""
    y = y.double().reshape(-1, 32)
    M = y.shape[0]
    assert M % 512 == 0
    f = torch.stack(uvw(p.reshape(-1), t.reshape(-1)), 1)                      # [M, 3]
    if absolute:
        f, y = f.abs(), y.abs()
    per = torch.cat([torch.einsum("wpk,wpc->wkc", f.reshape(-1, 512, 3), y.reshape(-1, 512, 32)).reshape(-1, 96),
                     f.reshape(-1, 512, 3).sum(1), torch.zeros(M // 512, 1, dtype=torch.float64)], 1)
    order = window_order(M // 512, win_pf, rev) if order is None else order
    return torch.stack([per[ws].sum(0) for ws in order])


def wsum_grad(rows, sums, inv_total, bce_w, gscale, absolute=False):
    """head_wsum_grad: rows [nr, 100] -> gw [32], gb [1]"""
    a, bb = dice_scalars(sums.double())
    c = torch.stack([a * gscale, bb * gscale, torch.as_tensor(bce_w * inv_total * gscale, dtype=torch.float64)])
    s = rows.double().sum(0)
    if absolute:
        c, s = c.abs(), rows.double().abs().sum(0)
    return (c[:, None] * s[:96].reshape(3, 32)).sum(0), (c * s[96:99]).sum().reshape(1)


# ---------------------------------------------------------------------- operands, guard
def dyadic_prob(seed, shape, pbits):
    """k / 2^pbits, k uniform in [1, 2^pbits - 1]"""
    return X.ints(seed, shape, 1, (1 << pbits) - 1) / float(1 << pbits)


def targets(seed, shape, density=0.4):
    return X.ints(seed, shape, 1, 1, density)


def dyadic_sums(s=1.25):
    """2 I + 1 = 4 and St + Sp + 1 = 4: a = -1/2, bb = 1/4 exactly (fp32 divisions of powers of two)"""
    return torch.tensor([1.5, s, 3.0 - s, 0.0], dtype=torch.float64)


def dlogit_frac_bits(pbits, inv_total, bce_w, gscale):
    """Resolution of the dyadic dlogit: the Dice term is a multiple of 2^-(2 + 2 pbits), the
    BCE term of bce_w inv_total 2^-pbits; both scaled by the loss scale (powers of two)."""
    fb = 2 + 2 * pbits
    if bce_w:
        l = math.log2(bce_w * inv_total)
        assert l == int(l), "bce_w * inv_total must be a power of two"
        fb = max(fb, pbits - int(l))
    g = math.log2(gscale)
    assert g == int(g), "the loss scale must be a power of two"
    return fb - int(g)


def require_exact_dyadic(abs_bound, frac_bits):
    """`abs_bound`: the reference on absolute values; 2^-frac_bits: the common resolution of
    its terms.  Every partial sum is then an integer multiple of 2^-frac_bits below 2^24 of
    them: exact in fp32 in any order."""
    b = float(torch.as_tensor(abs_bound).abs().max())
    assert b * 2.0 ** frac_bits < X.EXACT, (
        "case leaves the exact regime: sum of |terms| up to %.4g at resolution 2^-%d >= 2^24" % (b, frac_bits))
    return b


def centring_bias(z):
    """[P, K] logits without bias -> the bias (a multiple of 1/64 per class) that puts their
    median at 0: activations are non-negative, so the raw logits of a class lean to one side."""
    return -(z.double().median(0).values * 64).round() / 64.0


def on_grid(t, frac_bits):
    s = t.double() * 2.0 ** frac_bits
    return bool(torch.equal(s, s.round()))


# -------------------------------------------------------------------------------- cases
PBITS = 4                       # prob = k / 16
WMAX = 15                       # |head weight| (integers)
# fp16 keeps 11 bits: prob = k / 64 and |w| <= 31 so that dlogit w carries up to 15
WIDE = {"fp16": (6, 31)}
XMAX = 8                        # head input: integers in [0, 8], 60 % positive


@functools.lru_cache(maxsize=None)
def bwd_case(P, Cc, K, bce_w, gscale, inv_total, dtype="bf16"):
    """head_bwd / head_mc_bwd / head_dy on dyadic operands."""
    key = ("head_bwd", P, Cc, K, bce_w, gscale, inv_total, dtype)
    pbits, wmax = WIDE.get(dtype, (PBITS, WMAX))
    x = X.nonneg(X.seed_of(key, "x"), (P, Cc), XMAX, 0.6)
    W = X.ints(X.seed_of(key, "w"), (Cc, K), -wmax, wmax)
    p = dyadic_prob(X.seed_of(key, "p"), (P, K), pbits)
    t = targets(X.seed_of(key, "t"), (P, K))
    sums = dyadic_sums()
    dz, dx, gw, gb = head_backward(x, W, p, t, sums, inv_total, bce_w, gscale)
    bound = max(v.max().item() for v in head_grads(x, W.abs(), dz.abs()))
    return Case(ops=dict(x=x, W=W, p=p, t=t, sums=sums), ref=dict(dz=dz, dx=dx.contiguous(), gw=gw, gb=gb),
                bound=bound, frac_bits=dlogit_frac_bits(pbits, inv_total, bce_w, gscale), dtype=dtype, rounds=True,
                scal=(inv_total, bce_w, gscale))


@functools.lru_cache(maxsize=None)
def onload_case(N, H, Wd, Cy, bce_w, gscale, inv_total):
    """Head-on-load: dY = dlogit w (x > 0) of a 32-channel head input formed where the 3x3
    data gradient and the weight gradient of the head-input conv consume it.  The kernels
    round dY to 16 bits before the MFMAs (head_grad.h: "rounded exactly like head_bwd's
    stored gradient"): dx = RNE(conv_dgrad(RNE(dY), wt) (act > 0)), gw = conv_wgrad([act], RNE(dY))."""
    key = ("head_onload", N, H, Wd, Cy, bce_w, gscale, inv_total)
    sp = (N, H, Wd)
    x = X.nonneg(X.seed_of(key, "x"), sp + (32,), XMAX, 0.6)
    w = X.ints(X.seed_of(key, "w"), (32,), -WMAX, WMAX)
    p = dyadic_prob(X.seed_of(key, "p"), sp, PBITS)
    t = targets(X.seed_of(key, "t"), sp)
    sums = dyadic_sums()
    dz = dlogit(p, t, sums, inv_total, bce_w, gscale)
    dy64 = (dz[..., None] * w * (x > 0)).contiguous()
    dys = X.rne(dy64, "bf16").double()
    wt = X.ints(X.seed_of(key, "wt"), (3, 3, Cy, 32), -4, 4)
    act = X.nonneg(X.seed_of(key, "act"), sp + (Cy,), XMAX, 0.6)
    dx = (X.conv_dgrad_ref(dys, wt) * (act > 0)).contiguous()
    gw, gb = X.conv_wgrad_ref([act], dys)
    bw, bb = X.conv_wgrad_ref([act], dys.abs())
    bound = max(X.conv_dgrad_ref(dys.abs(), wt.abs()).max().item(), bw.max().item(), bb.max().item())
    return Case(ops=dict(x=x, w=w, p=p, t=t, sums=sums, wt=wt, act=act), ref=dict(dz=dz, dy=dy64, dx=dx, gw=gw, gb=gb),
                bound=bound, frac_bits=dlogit_frac_bits(PBITS, inv_total, bce_w, gscale), dtype="bf16", rounds=True,
                scal=(inv_total, bce_w, gscale))


@functools.lru_cache(maxsize=None)
def wsum_grad_case(nrows):
    """head_wsum_grad alone: hand-built rows of multiples of 1/8 (the serial loop up to 256
    rows, the 256-wide tree beyond), dyadic scalars."""
    key = ("wsum_grad", nrows)
    rows = X.ints(X.seed_of(key, "rows"), (nrows, 100), -64, 64) / 8.0
    rows[:, 99] = 0
    sums = dyadic_sums()
    scal = (2.0 ** -6, 0.5, 4.0)
    gw, gb = wsum_grad(rows, sums, *scal)
    bw, bb = wsum_grad(rows, sums, *scal, absolute=True)
    # rows: 2^-3; scalars a gs = -2, bb gs = 1, bce_w inv_total gs = 2^-5
    return Case(ops=dict(rows=rows, sums=sums), ref=dict(gw=gw, gb=gb), bound=max(bw.max().item(), bb.max().item()),
                frac_bits=8, dtype="fp32", rounds=False, scal=scal)


def fused_geometry(N, H):
    return (N, 1, H, 128, 32, 0, 32, 0)


@functools.lru_cache(maxsize=None)
def fused_case(N, H, win_pf, rev, wmax64=0):
    """The persistent fused-head forward with the Mask weight sums (head_ws): the conv of
    X.fwd_case(.., small=True), head weights multiples of 1/64 (wmax64 = 0: weights and bias
    zero, logit 0, p = 1/2: u = t / 4, v = 1 / 4, w = 1 / 2 - t exactly)."""
    key = ("head_fused", N, H, win_pf, rev, wmax64)
    conv = X.fwd_case(N, 1, H, 128, 32, 0, 32, "bf16", True, True)
    y = conv.ref["y"].reshape(-1, 32)                                 # |y| <= 64: stored without rounding
    M = y.shape[0]
    hw = X.ints(X.seed_of(key, "hw"), (32,), -wmax64, wmax64) / 64.0
    hb = centring_bias(y @ hw[:, None])
    t = targets(X.seed_of(key, "t"), (M,))
    z = y @ hw + hb
    p = sigmoid64(z)
    rows = ws_rows(y, p, t, win_pf, rev)
    rows_abs = ws_rows(y, p, t, win_pf, rev, absolute=True)
    return Case(ops=dict(conv=conv, hw=hw, hb=hb, t=t), ref=dict(y=y, z=z, p=p, rows=rows, rows_abs=rows_abs),
                bound=max(rows_abs.max().item(), (y.abs() @ hw.abs() + hb.abs()).max().item()),
                frac_bits=2 if wmax64 == 0 else 6, dtype="bf16", rounds=False)


@functools.lru_cache(maxsize=None)
def fused3d_case(N, D, H, wmax64):
    """3D: the 128-wide chunk-pipelined fused-head window, one 512-pixel window per workgroup
    (window xcd_remap(b) in row b)."""
    key = ("head_fused3d", N, D, H, wmax64)
    conv = X.fwd_case(N, D, H, 128, 32, 0, 32, "bf16", True, True)
    y = conv.ref["y"].reshape(-1, 32)                                 # integers below 256: stored without rounding
    M = y.shape[0]
    hw = X.ints(X.seed_of(key, "hw"), (32,), -wmax64, wmax64) / 64.0
    hb = centring_bias(y @ hw[:, None])
    t = targets(X.seed_of(key, "t"), (M,))
    z = y @ hw + hb
    p = sigmoid64(z)
    # head_dy from the forward's ReLU bits: dyadic operands of its own (integer weights)
    wi = X.ints(X.seed_of(key, "wi"), (32, 1), -WMAX, WMAX)
    pd = dyadic_prob(X.seed_of(key, "pd"), (M, 1), PBITS)
    scal = (INV_TOTAL, 0.5, 4.0)
    dz, dx, _, _ = head_backward(y, wi, pd, t[:, None], dyadic_sums(), *scal)
    order = window_order_cp(M // 512)
    return Case(ops=dict(conv=conv, hw=hw, hb=hb, t=t, wi=wi, pd=pd, sums=dyadic_sums()),
                ref=dict(y=y, z=z, p=p, rows=ws_rows(y, p, t, 1, 0, order=order),
                         rows_abs=ws_rows(y, p, t, 1, 0, absolute=True, order=order), dz=dz, dx=dx.contiguous()),
                bound=(y.abs() @ hw.abs() + hb.abs()).max().item(), frac_bits=6, dtype="bf16", rounds=False, scal=scal,
                dy_bound=(dz.abs() @ wi.abs().t()).max().item(), dy_frac_bits=dlogit_frac_bits(PBITS, *scal))


@functools.lru_cache(maxsize=None)
def finish_half_case(P, with_t=True):
    """head_finish at logit 0: prob exactly 1/2, so I = count / 2, Sp = P / 2 exactly."""
    t = targets(X.seed_of("finish_half", P), (P,)) if with_t else None
    z = torch.zeros(P, dtype=torch.float64)
    sums = loss_sums(z, t)
    return Case(ops=dict(z=z, t=t), ref=dict(p=torch.full((P,), 0.5, dtype=torch.float64), sums=sums,
                                             terms=sum_terms(z, t)),
                bound=float(P), frac_bits=1, dtype="bf16", rounds=False)


@functools.lru_cache(maxsize=None)
def finish_case(P):
    """head_finish on dyadic logits (multiples of 1/64) spread uniformly over [-6, 6]."""
    z = X.ints(X.seed_of("finish", P, "z"), (P,), -384, 384) / 64.0
    t = targets(X.seed_of("finish", P, "t"), (P,))
    return Case(ops=dict(z=z, t=t), ref=dict(p=sigmoid64(z), sums=loss_sums(z, t), terms=sum_terms(z, t)), bound=6.0,
                frac_bits=6, dtype="bf16", rounds=False)


# |W| <= FWD_WMAX64[C] / 64 with x in [0, 3] (half of them positive) spreads the logits over about +-6
FWD_WMAX64 = {16: 44, 32: 30, 64: 20}


@functools.lru_cache(maxsize=None)
def fwd_case(P, Cc, K):
    """head_fwd / head_mc_fwd: integer activations, weights and bias multiples of 1/64: the fp32
    logit is exact, the sigmoid, the BCE and the sums carry the error."""
    key = ("head_fwd", P, Cc, K)
    x = X.nonneg(X.seed_of(key, "x"), (P, Cc), 3, 0.5)
    W = X.ints(X.seed_of(key, "w"), (Cc, K), -FWD_WMAX64[Cc], FWD_WMAX64[Cc]) / 64.0
    b = centring_bias(x @ W)
    t = targets(X.seed_of(key, "t"), (P, K))
    z, p, sums = head_forward(x, W, b, t)
    return Case(ops=dict(x=x, W=W, b=b, t=t), ref=dict(z=z, p=p, sums=sums, terms=sum_terms(z, t)),
                bound=(x @ W.abs() + b.abs()).max().item(), frac_bits=6, dtype="bf16", rounds=False)


# The cases tests/test_gpu_head_exact.py launches.
INV_TOTAL = 2.0 ** -6            # an argument of the backward kernels: need not be 1 / P
# head_bwd, K = 1: (P, C, bce_w, loss scale, scale through the device pointer, dtype)
BWD_K1 = [(1001, 16, 0.0, 4.0, False, "bf16"), (1001, 16, 0.5, 8.0, True, "bf16"),
          (1001, 32, 0.0, 8.0, True, "bf16"), (1001, 32, 0.5, 4.0, False, "bf16"),
          (4096, 64, 0.0, 4.0, False, "bf16"), (4096, 64, 0.5, 8.0, True, "bf16"),
          (1001, 32, 0.5, 8.0, True, "fp16")]
# head_mc: (P, C, K, bce_w, loss scale, device pointer)
BWD_MC = [(1001, 32, 2, 0.5, 4.0, False), (1001, 32, 3, 0.0, 8.0, True), (1001, 64, 4, 0.5, 8.0, True)]
# head_dy: (P, C, bce_w, loss scale, device pointer)
HEAD_DY = [(1001, 32, 0.5, 4.0, False), (4096, 64, 0.0, 8.0, True)]
# head-on-load: (N, H, W, Cy, bce_w, loss scale, window variant of the data gradient)
ONLOAD = [(3, 16, 16, 32, 0.5, 2.0, {}), (2, 64, 64, 64, 0.0, 1.0, {}), (3, 8, 128, 32, 0.5, 2.0, dict(win_pf=5, rev=1))]
ONLOAD_SPLITS = (3, 7)
WSUM_GRAD_ROWS = (1, 7, 300)
FUSED_HALF = [(3, 8, 5, 0), (3, 8, 5, 1), (3, 128, 5, 0), (3, 128, 5, 1)]               # (N, H, win_pf, rev)
FINISH_HALF = (1, 3, 1001, 4096, 4 * 256 * 1024 + 1027, 4 * 256 * 4096 + 1027)
# (head_finish launches at most 4096 blocks of 256 threads x 4 pixels: only the last size runs a
# second grid-stride round)
FINISH = (1001, 4096)
HEAD_FWD = [(1001, 16, 1), (1001, 32, 1), (4096, 64, 1), (1001, 32, 2), (1001, 32, 3), (1001, 64, 4)]
FUSED_REAL = [(3, 8, 5, 1, 5), (3, 128, 5, 0, 5)]                                    # (..., |hw| max in 1/64)
CHAIN = (3, 128, 5, 0, 5)
FUSED_3D = (2, 3, 8, 3)                                                                # (N, D, H, |hw| max in 1/64)
FP16_BUILD = [k for k in BWD_K1 if k[5] == "fp16"]


def dyadic_cases():
    """(name, builder, 16-bit outputs) of every dyadic case"""
    out = []
    for (P, Cc, bw, gs, dev, dt) in BWD_K1:
        out.append(("head_bwd %s" % ((P, Cc, bw, gs, dt),), functools.partial(bwd_case, P, Cc, 1, bw, gs, INV_TOTAL, dt),
                    ("dx",)))
    for (P, Cc, K, bw, gs, dev) in BWD_MC:
        out.append(("head_mc_bwd %s" % ((P, Cc, K, bw, gs),), functools.partial(bwd_case, P, Cc, K, bw, gs, INV_TOTAL), ("dx",)))
    for (P, Cc, bw, gs, dev) in HEAD_DY:
        out.append(("head_dy %s" % ((P, Cc, bw, gs),), functools.partial(bwd_case, P, Cc, 1, bw, gs, INV_TOTAL), ("dx",)))
    for (N, H, Wd, Cy, bw, gs, var) in ONLOAD:
        out.append(("head on load %s" % ((N, H, Wd, Cy, bw, gs),), functools.partial(onload_case, N, H, Wd, Cy, bw, gs, INV_TOTAL),
                    ("dy", "dx")))
    return out


def target_cases():
    """(name, targets) of every case, dyadic or not"""
    out = [(n, lambda m=m: m().ops["t"]) for n, m, _ in dyadic_cases()]
    out += [("fused half %s" % (k,), lambda k=k: fused_case(*k).ops["t"]) for k in FUSED_HALF]
    out += [("fused %s" % (k,), lambda k=k: fused_case(*k).ops["t"]) for k in FUSED_REAL + [CHAIN]]
    out += [("fused 3d", lambda: fused3d_case(*FUSED_3D).ops["t"])]
    out += [("finish half %d" % P, lambda P=P: finish_half_case(P).ops["t"]) for P in FINISH_HALF if P >= 1001]
    out += [("finish %d" % P, lambda P=P: finish_case(P).ops["t"]) for P in FINISH]
    out += [("head_fwd %s" % (k,), lambda k=k: fwd_case(*k).ops["t"]) for k in HEAD_FWD]
    return out

"""512-pixel windows of the 64-channel row-window tile on 16-wide rows (win_bm2 bit 2,
conv_win.h win_b512_eligible, conv_win_kernel<16, 64, 512, ..>): a window is two whole 16 x 16
images, and the two halo fragments that would cross the seam between them are read from the
halo image's zero rows.  Every output element keeps the 256-pixel window's operands and
accumulation order, so each launch must write exactly what win_bm2 = 3 writes -- forward with
bias + ReLU + bits, the fused max-pool, concat sources, the generic epilogue with dropout,
data gradients with 1-bit / 16-bit masks and the pool route, the reversed walk.  The grid
tells which kernel ran: the 512-pixel launch has half the workgroups.  An odd image count
keeps 256 pixels.  Seam cases: two images against each image alone, and a zero image beside
a random one (no tap may leak across the seam in either direction)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import C, _pack_bits, pack_dgrad, pack_fwd, ptr, stream
from test_gpu_win512 import _guarded, _guards_intact

pytestmark = pytest.mark.gpu
H = 16
OFF, ON = 3, 7         # win_bm2: the 32 / 64-wide bits alone, and with bit 2


def _geo(N):
    return dict(N=N, OH=H, OW=H, IH=H, IW=H, KH=3, KW=3, pad=1, win_cp=1)


def _grids(d, halves):
    g0, g1 = C().conv_fwd_grid(dict(d, win_bm2=OFF)), C().conv_fwd_grid(dict(d, win_bm2=ON))
    assert g0 == d["N"] * H * H // 256 * (d["Cout"] // 64), g0
    assert g1 == (g0 // 2 if halves else g0), (g0, g1)


def _run(d, outs, bm2):
    for t in outs:
        t.fill_(float("nan") if t.is_floating_point() else 0)
    C().conv_fwd(dict(d, win_bm2=bm2), stream())
    torch.cuda.synchronize()
    return [t.clone() for t in outs]


def _ab(d, outs, halves=True):
    """Run conv dict `d` with win_bm2 = 3 and 7 on fresh NaN-filled outputs: the two-image
    launch has half the workgroups (`halves` False: the same grid, the 256-pixel path) and
    every output is bit-identical.  Returns the on arm's outputs."""
    _grids(d, halves)
    res = [_run(d, outs, bm2) for bm2 in (OFF, ON)]
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t.float()).all() for t in res[1] if t.is_floating_point())
    return res[1]


def _fwd_dict(dev, N, C1, C2, Cout, pool, rev=0, seed=231, x1=None):
    """Forward conv dict with bias + ReLU + bits (+ fused pool), its outputs and operands."""
    torch.manual_seed(seed)
    # (weights and bias first: they do not depend on N or on a given x1)
    w = (torch.randn(3, 3, C1 + C2, Cout, device=dev) * 0.05).bfloat16()
    b = torch.randn(Cout, device=dev) * 0.1
    if x1 is None:
        x1 = F.relu(torch.randn(N, H, H, C1, device=dev)).bfloat16()
    y = torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16)
    bits = torch.empty(N * H * H * Cout // 8, device=dev, dtype=torch.uint8)
    keep = [x1, pack_fwd(w), b]
    d = dict(_geo(N), C1=C1, C2=C2, src1=ptr(x1), wgt=ptr(keep[1]), bias=ptr(b), Cout=Cout, relu=1,
             dst1=ptr(y), relu_bits=ptr(bits), rev=rev)
    outs = [y, bits]
    if C2:
        keep.append(F.relu(torch.randn(N, H, H, C2, device=dev)).bfloat16())
        d["src2"] = ptr(keep[-1])
    if pool:
        pooled = torch.empty(N, H // 2, H // 2, Cout, device=dev, dtype=torch.bfloat16)
        codes = torch.empty(N * (H // 2) ** 2 * Cout // 8, device=dev, dtype=torch.int32)
        d.update(pool_dst=ptr(pooled), pool_code=ptr(codes))
        outs += [pooled, codes]
    return d, outs, keep


def _fwd(dev, N, C1, C2, Cout, pool, rev=0, halves=True):
    d, outs, keep = _fwd_dict(dev, N, C1, C2, Cout, pool, rev)
    got = _ab(d, outs, halves)
    assert got[0].float().abs().sum() > 0 and got[1].any()
    assert torch.equal(got[1], _pack_bits(got[0]).reshape(-1))
    if pool:
        assert torch.equal(got[2], F.max_pool2d(got[0].float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).bfloat16())


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("Cout", [64, 128])
@pytest.mark.parametrize("Cin", [64, 128])
def test_w16_forward(cuda_dev, Cin, Cout, pool):
    """N = 6: three two-image windows, not a multiple of the XCD count."""
    _fwd(cuda_dev, 6, Cin, 0, Cout, pool)


def test_w16_forward_concat(cuda_dev):
    _fwd(cuda_dev, 6, 64, 64, 64, 0)


def test_w16_forward_rev(cuda_dev):
    _fwd(cuda_dev, 6, 64, 0, 128, 1, rev=1)


def test_w16_forward_generic_dropout(cuda_dev):
    """Dropout after the ReLU: the generic epilogue, its keep hash addressed by global element."""
    torch.manual_seed(232)
    dev, N, Cin, Cout = cuda_dev, 6, 128, 64
    x = torch.randn(N, H, H, Cin, device=dev).bfloat16()
    wp = pack_fwd((torch.randn(3, 3, Cin, Cout, device=dev) * 0.05).bfloat16())
    b = torch.randn(Cout, device=dev) * 0.1
    y = torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16)
    got = _ab(dict(_geo(N), C1=Cin, src1=ptr(x), wgt=ptr(wp), bias=ptr(b), Cout=Cout, dst1=ptr(y), relu=1,
                   drop_rate=0.25, seed=3, salt=5), [y])
    zero = (got[0].float() == 0).float().mean().item()
    assert 0.5 < zero < 0.75, zero          # ReLU zeros about half, dropout a quarter of the rest


def _dgrad_dict(dev, N, Co, Ci, mode, rev=0, dy=None):
    """Data gradient dY [Co] -> dX [Ci] of a 3x3 conv Ci -> Co; mode: "bits" (1-bit ReLU mask),
    "act" (16-bit activation as the mask), "route" (1-bit mask + the fused pool backward)."""
    torch.manual_seed(233)
    act = F.relu(torch.randn(N, H, H, Ci, device=dev)).bfloat16()
    w = (torch.randn(3, 3, Ci, Co, device=dev) * 0.05).bfloat16()
    if dy is None:
        dy = torch.randn(N, H, H, Co, device=dev).bfloat16()
    dx = torch.empty(N, H, H, Ci, device=dev, dtype=torch.bfloat16)
    keep = dict(src1=dy, wgt=pack_dgrad(w), act=act)
    d = dict(_geo(N), C1=Co, src1=ptr(dy), wgt=ptr(keep["wgt"]), Cout=Ci, dst1=ptr(dx), rev=rev)
    if mode == "act":
        keep["mask1"] = act
        d.update(mask1=ptr(act), mask_bits=0)
    else:
        keep["mask1"] = _pack_bits(act)
        d.update(mask1=ptr(keep["mask1"]), mask_bits=1)
    if mode == "route":
        pooled = torch.empty(N, H // 2, H // 2, Ci, device=dev, dtype=torch.bfloat16)
        keep["pool_code"] = torch.zeros(N * (H // 2) ** 2 * Ci // 8, device=dev, dtype=torch.int32)
        C().generic("pool_fwd", [ptr(act), ptr(pooled), ptr(keep["pool_code"])], [N, 1, H, H, Ci, 0], [], stream())
        keep["route_gy"] = torch.randn(N, H // 2, H // 2, Ci, device=dev).bfloat16()
        d.update(route_gy=ptr(keep["route_gy"]), pool_code=ptr(keep["pool_code"]))
    return d, dx, keep


@pytest.mark.parametrize("mode,rev", [("bits", 0), ("act", 0), ("route", 0), ("bits", 1)])
def test_w16_dgrad(cuda_dev, mode, rev):
    d, dx, keep = _dgrad_dict(cuda_dev, 6, 128, 64, mode, rev)
    got = _ab(d, [dx])
    assert got[0].float().abs().sum() > 0
    # the mask took effect: no gradient where the activation is not positive (route: nor a pool argmax)
    if mode != "route":
        assert (got[0].float()[keep["act"].float() <= 0] == 0).all()


def test_w16_dgrad_two_destinations(cuda_dev):
    """dY -> (upsampled half, skip half) with one bit mask each and a rescale on the second."""
    torch.manual_seed(234)
    dev, N, C1, C2, Co = cuda_dev, 6, 64, 64, 128
    m1 = torch.randn(N, H, H, C1, device=dev).bfloat16()
    m2 = torch.randn(N, H, H, C2, device=dev).bfloat16()
    wdg = pack_dgrad((torch.randn(3, 3, C1 + C2, Co, device=dev) * 0.05).bfloat16())
    dy = torch.randn(N, H, H, Co, device=dev).bfloat16()
    b1, b2 = _pack_bits(m1), _pack_bits(m2)
    d1 = torch.empty(N, H, H, C1, device=dev, dtype=torch.bfloat16)
    d2 = torch.empty(N, H, H, C2, device=dev, dtype=torch.bfloat16)
    got = _ab(dict(_geo(N), C1=Co, src1=ptr(dy), wgt=ptr(wdg), Cout=C1 + C2, D1=C1, dst1=ptr(d1), dst2=ptr(d2),
                   mask1=ptr(b1), mask2=ptr(b2), mask_bits=3, mask_scale2=1.25), [d1, d2])
    assert got[0].float().abs().sum() > 0 and got[1].float().abs().sum() > 0


# ------------------------------------------------------------------------------ seam
@pytest.mark.parametrize("Cin,Cout,pool", [(64, 64, 1), (128, 128, 0)])
def test_w16_seam_forward_pair_equals_each_image_alone(cuda_dev, Cin, Cout, pool):
    """N = 2 (one two-image window) against each image run alone: N = 1 can only take the
    256-pixel path."""
    d, outs, keep = _fwd_dict(cuda_dev, 2, Cin, 0, Cout, pool)
    _grids(d, True)
    pair = _run(d, outs, ON)
    x = keep[0]
    for i in range(2):
        xi = x[i:i + 1].contiguous()
        d1, outs1, keep1 = _fwd_dict(cuda_dev, 1, Cin, 0, Cout, pool, x1=xi)     # (same seed: same weights, bias)
        _grids(d1, False)
        one = _run(d1, outs1, ON)
        for a, b in zip(pair, one):
            n = b.numel()
            assert torch.equal(a.reshape(-1)[i * n:(i + 1) * n], b.reshape(-1)), i


def test_w16_seam_dgrad_pair_equals_each_image_alone(cuda_dev):
    d, dx, keep = _dgrad_dict(cuda_dev, 2, 128, 64, "bits")
    _grids(d, True)
    pair = _run(d, [dx], ON)[0]
    for i in range(2):
        dyi = keep["src1"][i:i + 1].contiguous()
        mi = _pack_bits(keep["act"][i:i + 1].contiguous())
        dxi = torch.empty(1, H, H, 64, device=cuda_dev, dtype=torch.bfloat16)
        d1 = dict(d, N=1, src1=ptr(dyi), mask1=ptr(mi), dst1=ptr(dxi))
        _grids(d1, False)
        assert torch.equal(pair[i:i + 1], _run(d1, [dxi], ON)[0]), i


@pytest.mark.parametrize("zero", [0, 1])
def test_w16_seam_zero_image_sees_bias_only(cuda_dev, zero):
    """One image of the window all zeros, the other random: the zero image's output is
    ReLU(bias) everywhere -- a tap leaking across the seam (A's last row into B's first, or
    B's first row into A's last) would add the neighbour's pixels."""
    dev, Cin, Cout = cuda_dev, 64, 64
    torch.manual_seed(235)
    x = (torch.randn(2, H, H, Cin, device=dev).abs() + 1).bfloat16()     # every pixel well away from zero
    x[zero] = 0
    d, outs, keep = _fwd_dict(dev, 2, Cin, 0, Cout, 0, x1=x)
    got = _ab(d, outs)
    want = F.relu(keep[2]).bfloat16().expand(H, H, Cout)
    assert torch.equal(got[0][zero], want)
    assert not torch.equal(got[0][1 - zero], want)
    # the same through the data gradient: a zero dY image gives a zero dX image
    dy = torch.randn(2, H, H, 128, device=dev).bfloat16()
    dy[zero] = 0
    dd, dx, _ = _dgrad_dict(dev, 2, 128, 64, "act", dy=dy)
    gd = _ab(dd, [dx])[0]
    assert (gd[zero] == 0).all() and gd[1 - zero].float().abs().sum() > 0


# -------------------------------------------------------------------------- fallback
def test_w16_odd_image_count_keeps_256(cuda_dev):
    _fwd(cuda_dev, 3, 64, 0, 64, 1, halves=False)
    d, dx, _ = _dgrad_dict(cuda_dev, 3, 128, 64, "route")
    _ab(d, [dx], halves=False)


# ---------------------------------------------------------------------------- bounds
def _bounds(d, ins, outs):
    """`d` holds tensors for the operand keys `ins` and output keys `outs`.  Reference: the
    256-pixel launch on ordinary allocations.  Then the two-image launch with every operand
    and output embedded in poison: outputs finite and equal to the reference, guards intact."""
    def ptrs(q, bm2):
        return dict({k: (ptr(v) if isinstance(v, torch.Tensor) else v) for k, v in q.items()}, win_bm2=bm2)

    def launch(q, bm2):
        C().conv_fwd(ptrs(q, bm2), stream())
        torch.cuda.synchronize()
    ref = dict(d)
    for k in outs:
        ref[k] = torch.full_like(d[k], float("nan")) if d[k].dtype.is_floating_point else torch.zeros_like(d[k])
    launch(ref, OFF)
    g, bufs = dict(d), {}
    for k in ins:
        g[k], bufs[k] = _guarded(d[k])
    for k in outs:
        g[k], bufs[k] = _guarded(d[k], fill=float("nan") if d[k].dtype.is_floating_point else 0)
    assert C().conv_fwd_grid(ptrs(g, ON)) * 2 == C().conv_fwd_grid(ptrs(g, OFF))
    launch(g, ON)
    for k in outs:
        if g[k].dtype.is_floating_point:
            assert torch.isfinite(g[k].float()).all(), k
        assert torch.equal(g[k], ref[k]), k
    for k, b in bufs.items():
        assert _guards_intact(b), k


def test_w16_bounds_forward_pool(cuda_dev):
    """Concat forward with bias + ReLU + bits and the fused max-pool."""
    torch.manual_seed(236)
    dev, N, C1, C2, Cout = cuda_dev, 6, 64, 64, 64
    d = dict(_geo(N), C1=C1, C2=C2, src1=F.relu(torch.randn(N, H, H, C1, device=dev)).bfloat16(),
             src2=F.relu(torch.randn(N, H, H, C2, device=dev)).bfloat16(),
             wgt=pack_fwd((torch.randn(3, 3, C1 + C2, Cout, device=dev) * 0.05).bfloat16()),
             bias=torch.randn(Cout, device=dev) * 0.1, Cout=Cout, relu=1,
             dst1=torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16),
             relu_bits=torch.empty(N * H * H * Cout // 8, device=dev, dtype=torch.uint8),
             pool_dst=torch.empty(N, H // 2, H // 2, Cout, device=dev, dtype=torch.bfloat16),
             pool_code=torch.empty(N * (H // 2) ** 2 * Cout // 8, device=dev, dtype=torch.int32))
    _bounds(d, ["src1", "src2", "wgt", "bias"], ["dst1", "relu_bits", "pool_dst", "pool_code"])


def test_w16_bounds_dgrad_route(cuda_dev):
    """Data gradient with the 1-bit mask and the pool route, reversed walk."""
    torch.manual_seed(237)
    dev, N, Co, Ci = cuda_dev, 6, 128, 64
    act = F.relu(torch.randn(N, H, H, Ci, device=dev)).bfloat16()
    pooled = torch.empty(N, H // 2, H // 2, Ci, device=dev, dtype=torch.bfloat16)
    codes = torch.zeros(N * (H // 2) ** 2 * Ci // 8, device=dev, dtype=torch.int32)
    C().generic("pool_fwd", [ptr(act), ptr(pooled), ptr(codes)], [N, 1, H, H, Ci, 0], [], stream())
    d = dict(_geo(N), C1=Co, src1=torch.randn(N, H, H, Co, device=dev).bfloat16(),
             wgt=pack_dgrad((torch.randn(3, 3, Ci, Co, device=dev) * 0.05).bfloat16()), Cout=Ci,
             dst1=torch.empty(N, H, H, Ci, device=dev, dtype=torch.bfloat16), mask1=_pack_bits(act), mask_bits=1,
             route_gy=torch.randn(N, H // 2, H // 2, Ci, device=dev).bfloat16(), pool_code=codes, rev=1)
    _bounds(d, ["src1", "wgt", "mask1", "route_gy", "pool_code"], ["dst1"])


# ------------------------------------------------------------------------ whole step
def test_w16_step_is_bit_identical(cuda_dev, monkeypatch):
    """One training step of the 128^2 model with win_bm2 = 3 against 7: loss sums,
    probabilities, the first layer's activation gradient and every parameter gradient."""
    from test_gpu_model import _setup
    outs = []
    for v in (OFF, ON):
        monkeypatch.setenv("UNET_ENGINE", "win_bm2=%d" % v)
        spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, batch_size=4, img_size=128, in_channels=4)
        e = nb.engine
        assert e.opts["win_bm2"] == v
        nb.fwd_bwd(x, y, seed=31)
        torch.cuda.synchronize()
        outs.append((nb.sums().cpu(), e.prob.clone(), e.bufs["d:conv1a"].clone(),
                     {k: fn.view(fn.grad, k).clone() for k, *_ in fn.entries}))
    (s0, p0, d0, g0), (s1, p1, d1, g1) = outs
    assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(d0, d1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k

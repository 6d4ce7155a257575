"""512-pixel windows of the 64-channel row-window tile (conv_win.h win_b512_eligible,
conv_win_b64_512.hip; win_bm2 bit 0 = 32-wide rows, bit 1 = 64-wide rows): every output
element accumulates chunk -> dw -> halo row -> dh whatever the window's row count, so each
launch must write exactly what the 256-pixel window writes (on 64-wide rows: what the
chunk-pipelined 256-pixel window writes) -- forward with bias + ReLU + bits, the fused
max-pool, concat sources, data gradients with 1-bit / 16-bit masks and the pool route, the
reversed walk, the space-to-depth source.  The grid tells which kernel ran: the 512-pixel
launch has half the workgroups.  Statistics epilogues, 16-wide rows and 3D keep 256 pixels."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import C, _pack_bits, pack_dgrad, pack_fwd, pad64, ptr, stream

pytestmark = pytest.mark.gpu
PAD = 1 << 14          # guard elements on each side (bounds cases)


def _geo(N, H):
    # (win_cp = 1: the off arm of 64-wide rows is the executor's, the chunk-pipelined window)
    return dict(N=N, OH=H, OW=H, IH=H, IW=H, KH=3, KW=3, pad=1, win_cp=1)


def _ab(d, outs, halves=True):
    """Run conv dict `d` with win_bm2 = 0 and 3 on fresh outputs; the 512-pixel launch has
    half the workgroups (`halves` False: the same grid, the 256-pixel path); every output
    must be bit-identical.  Returns the on arm's outputs."""
    g0, g1 = C().conv_fwd_grid(dict(d, win_bm2=0)), C().conv_fwd_grid(dict(d, win_bm2=3))
    px = d["N"] * d.get("OD", 1) * d["OH"] * d["OW"]
    assert g0 == px // 256 * (d["Cout"] // 64), (g0, px)
    assert g1 == (g0 // 2 if halves else g0), (g0, g1)
    res = []
    for bm2 in (0, 3):
        for t in outs:
            t.fill_(float("nan") if t.is_floating_point() else 0)
        C().conv_fwd(dict(d, win_bm2=bm2), stream())
        torch.cuda.synchronize()
        res.append([t.clone() for t in outs])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t.float()).all() for t in res[1] if t.is_floating_point())
    return res[1]


def _fwd(dev, N, H, C1, C2, Cout, pool, rev=0, seed=181):
    torch.manual_seed(seed)
    x1 = F.relu(torch.randn(N, H, H, C1, device=dev)).bfloat16()
    w = (torch.randn(3, 3, C1 + C2, Cout, device=dev) * 0.05).bfloat16()
    b = torch.randn(Cout, device=dev) * 0.1
    y = torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16)
    bits = torch.empty(N * H * H * Cout // 8, device=dev, dtype=torch.uint8)
    wp = pack_fwd(w)
    d = dict(_geo(N, H), C1=C1, C2=C2, src1=ptr(x1), wgt=ptr(wp), bias=ptr(b), Cout=Cout, relu=1,
             dst1=ptr(y), relu_bits=ptr(bits), rev=rev)
    outs = [y, bits]
    if C2:
        x2 = F.relu(torch.randn(N, H, H, C2, device=dev)).bfloat16()
        d["src2"] = ptr(x2)
    if pool:
        pooled = torch.empty(N, H // 2, H // 2, Cout, device=dev, dtype=torch.bfloat16)
        codes = torch.empty(N * (H // 2) ** 2 * Cout // 8, device=dev, dtype=torch.int32)
        d.update(pool_dst=ptr(pooled), pool_code=ptr(codes))
        outs += [pooled, codes]
    got = _ab(d, outs)
    assert got[0].float().abs().sum() > 0 and got[1].any()
    if pool:
        assert torch.equal(got[2], F.max_pool2d(got[0].float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).bfloat16())


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("Cout", [64, 128])
@pytest.mark.parametrize("Cin", [32, 64, 128])
def test_win512_forward_w32(cuda_dev, Cin, Cout, pool):
    """N = 3: six 512-pixel windows, not a multiple of the XCD count."""
    _fwd(cuda_dev, 3, 32, Cin, 0, Cout, pool)


def test_win512_forward_concat_w32(cuda_dev):
    _fwd(cuda_dev, 3, 32, 64, 64, 128, 0)


def test_win512_forward_rev_w32(cuda_dev):
    _fwd(cuda_dev, 3, 32, 64, 0, 128, 1, rev=1)


def test_win512_forward_pool_w64(cuda_dev):
    _fwd(cuda_dev, 2, 64, 64, 0, 64, 1)


def test_win512_forward_concat_w64(cuda_dev):
    _fwd(cuda_dev, 2, 64, 64, 64, 64, 0)


def _dgrad(dev, N, H, Co, Ci, mode, rev=0):
    """Data gradient dY [Co] -> dX [Ci] of a 3x3 conv Ci -> Co; mode: "bits" (1-bit ReLU mask),
    "act" (16-bit activation as the mask), "route" (1-bit mask + the fused pool backward)."""
    torch.manual_seed(182)
    act = F.relu(torch.randn(N, H, H, Ci, device=dev)).bfloat16()
    w = (torch.randn(3, 3, Ci, Co, device=dev) * 0.05).bfloat16()
    dy = torch.randn(N, H, H, Co, device=dev).bfloat16()
    dx = torch.empty(N, H, H, Ci, device=dev, dtype=torch.bfloat16)
    wdg = pack_dgrad(w)
    d = dict(_geo(N, H), C1=Co, src1=ptr(dy), wgt=ptr(wdg), Cout=Ci, dst1=ptr(dx), rev=rev)
    bits = _pack_bits(act)
    if mode == "act":
        d.update(mask1=ptr(act), mask_bits=0)
    else:
        d.update(mask1=ptr(bits), mask_bits=1)
    if mode == "route":
        pooled = torch.empty(N, H // 2, H // 2, Ci, device=dev, dtype=torch.bfloat16)
        codes = torch.zeros(N * (H // 2) ** 2 * Ci // 8, device=dev, dtype=torch.int32)
        C().generic("pool_fwd", [ptr(act), ptr(pooled), ptr(codes)], [N, 1, H, H, Ci, 0], [], stream())
        dpool = torch.randn(N, H // 2, H // 2, Ci, device=dev).bfloat16()
        d.update(route_gy=ptr(dpool), pool_code=ptr(codes))
    got = _ab(d, [dx])
    assert got[0].float().abs().sum() > 0
    # the mask took effect: no gradient where the activation is not positive (route: nor a pool argmax)
    if mode != "route":
        assert (got[0].float()[act.float() <= 0] == 0).all()


@pytest.mark.parametrize("mode,rev", [("bits", 0), ("act", 0), ("route", 0), ("bits", 1)])
def test_win512_dgrad_w32(cuda_dev, mode, rev):
    _dgrad(cuda_dev, 3, 32, 128, 64, mode, rev)


def test_win512_dgrad_route_w64(cuda_dev):
    _dgrad(cuda_dev, 2, 64, 64, 64, "route")


@pytest.mark.parametrize("N,H,K,O", [(3, 32, 128, 64), (2, 64, 64, 32)])
def test_win512_dgrad_s2d(cuda_dev, N, H, K, O):
    """Space-to-depth source (XF 4): the fine [N][2H][2W][O] gradient read as the coarse image with
    C1 = 4 O channels, structurally zero taps skipped."""
    torch.manual_seed(183)
    dz = torch.randn(N, 2 * H, 2 * H, O, device=cuda_dev).bfloat16()
    wg = pad64((torch.randn(K, 36 * O, device=cuda_dev) * 0.05).bfloat16())
    b = F.relu(torch.randn(N, H, H, K, device=cuda_dev)).bfloat16()
    bits = _pack_bits(b)
    db = torch.empty(N, H, H, K, device=cuda_dev, dtype=torch.bfloat16)
    got = _ab(dict(_geo(N, H), C1=4 * O, s2d=O, src1=ptr(dz), wgt=ptr(wg), Cout=K, dst1=ptr(db), mask1=ptr(bits),
                   mask_bits=1), [db])
    assert got[0].float().abs().sum() > 0


# ---------------------------------------------------------------------------- bounds
def _guarded(t, fill=None):
    """(view, buffer): a copy of `t` (or, with `fill`, a `fill`-valued tensor of its shape) in the
    middle of a buffer whose PAD elements on each side are poison (NaN / all-ones bits)."""
    n = t.numel()
    poison = float("nan") if t.dtype.is_floating_point else (255 if t.dtype == torch.uint8 else -1)
    buf = torch.full((n + 2 * PAD,), poison, dtype=t.dtype, device=t.device)
    if fill is None:
        buf[PAD:PAD + n] = t.reshape(-1)
    else:
        buf[PAD:PAD + n] = fill
    return buf[PAD:PAD + n].view(t.shape), buf


def _guards_intact(buf):
    for g in (buf[:PAD], buf[-PAD:]):
        if buf.dtype.is_floating_point:
            if not torch.isnan(g).all():
                return False
        elif not (g == (255 if buf.dtype == torch.uint8 else -1)).all():
            return False
    return True


def _bounds(d, ins, outs):
    """`d` holds tensors for the operand keys `ins` and output keys `outs`.  Reference: the
    256-pixel launch on ordinary allocations.  Then the 512-pixel launch with every operand
    and output embedded in poison: outputs finite and equal to the reference, guards intact."""
    def ptrs(q, bm2):
        return dict({k: (ptr(v) if isinstance(v, torch.Tensor) else v) for k, v in q.items()}, win_bm2=bm2)

    def launch(q, bm2):
        C().conv_fwd(ptrs(q, bm2), stream())
        torch.cuda.synchronize()
    ref = dict(d)
    for k in outs:
        ref[k] = torch.full_like(d[k], float("nan")) if d[k].dtype.is_floating_point else torch.zeros_like(d[k])
    launch(ref, 0)
    g, bufs = dict(d), {}
    for k in ins:
        g[k], bufs[k] = _guarded(d[k])
    for k in outs:
        g[k], bufs[k] = _guarded(d[k], fill=float("nan") if d[k].dtype.is_floating_point else 0)
    assert C().conv_fwd_grid(ptrs(g, 3)) * 2 == C().conv_fwd_grid(ptrs(g, 0))
    launch(g, 3)
    for k in outs:
        if g[k].dtype.is_floating_point:
            assert torch.isfinite(g[k].float()).all(), k
        assert torch.equal(g[k], ref[k]), k
    for k, b in bufs.items():
        assert _guards_intact(b), k


def test_win512_bounds_dgrad_route_w32(cuda_dev):
    """32-wide rows: concat-free data gradient with the 1-bit mask and the pool route, reversed walk."""
    torch.manual_seed(184)
    dev, N, H, Co, Ci = cuda_dev, 3, 32, 128, 64
    act = F.relu(torch.randn(N, H, H, Ci, device=dev)).bfloat16()
    pooled = torch.empty(N, H // 2, H // 2, Ci, device=dev, dtype=torch.bfloat16)
    codes = torch.zeros(N * (H // 2) ** 2 * Ci // 8, device=dev, dtype=torch.int32)
    C().generic("pool_fwd", [ptr(act), ptr(pooled), ptr(codes)], [N, 1, H, H, Ci, 0], [], stream())
    d = dict(_geo(N, H), C1=Co, src1=torch.randn(N, H, H, Co, device=dev).bfloat16(),
             wgt=pack_dgrad((torch.randn(3, 3, Ci, Co, device=dev) * 0.05).bfloat16()), Cout=Ci,
             dst1=torch.empty(N, H, H, Ci, device=dev, dtype=torch.bfloat16), mask1=_pack_bits(act), mask_bits=1,
             route_gy=torch.randn(N, H // 2, H // 2, Ci, device=dev).bfloat16(), pool_code=codes, rev=1)
    _bounds(d, ["src1", "wgt", "mask1", "route_gy", "pool_code"], ["dst1"])


def test_win512_bounds_forward_pool_w64(cuda_dev):
    """64-wide rows: concat forward with bias + ReLU + bits and the fused max-pool."""
    torch.manual_seed(185)
    dev, N, H, C1, C2, Cout = cuda_dev, 2, 64, 64, 64, 64
    d = dict(_geo(N, H), C1=C1, C2=C2, src1=F.relu(torch.randn(N, H, H, C1, device=dev)).bfloat16(),
             src2=F.relu(torch.randn(N, H, H, C2, device=dev)).bfloat16(),
             wgt=pack_fwd((torch.randn(3, 3, C1 + C2, Cout, device=dev) * 0.05).bfloat16()),
             bias=torch.randn(Cout, device=dev) * 0.1, Cout=Cout, relu=1,
             dst1=torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16),
             relu_bits=torch.empty(N * H * H * Cout // 8, device=dev, dtype=torch.uint8),
             pool_dst=torch.empty(N, H // 2, H // 2, Cout, device=dev, dtype=torch.bfloat16),
             pool_code=torch.empty(N * (H // 2) ** 2 * Cout // 8, device=dev, dtype=torch.int32))
    _bounds(d, ["src1", "src2", "wgt", "bias"], ["dst1", "relu_bits", "pool_dst", "pool_code"])


# -------------------------------------------------------------------------- negative
def test_win512_keeps_256_on_16_wide_rows(cuda_dev):
    torch.manual_seed(186)
    N, H, Cin, Cout = 4, 16, 64, 64
    x = F.relu(torch.randn(N, H, H, Cin, device=cuda_dev)).bfloat16()
    w = (torch.randn(3, 3, Cin, Cout, device=cuda_dev) * 0.05).bfloat16()
    b = torch.randn(Cout, device=cuda_dev) * 0.1
    y = torch.empty(N, H, H, Cout, device=cuda_dev, dtype=torch.bfloat16)
    wp = pack_fwd(w)
    _ab(dict(_geo(N, H), C1=Cin, src1=ptr(x), wgt=ptr(wp), bias=ptr(b), Cout=Cout, relu=1, dst1=ptr(y)), [y],
        halves=False)


@pytest.mark.parametrize("H", [32, 64])
def test_win512_keeps_256_with_statistics(cuda_dev, H):
    """One statistics row per 256-pixel window: the row count must not change."""
    torch.manual_seed(187)
    N, Cin, Cout = 2, 64, 64
    x = torch.randn(N, H, H, Cin, device=cuda_dev).bfloat16()
    w = (torch.randn(3, 3, Cin, Cout, device=cuda_dev) * 0.05).bfloat16()
    b = torch.randn(Cout, device=cuda_dev) * 0.1
    y = torch.empty(N, H, H, Cout, device=cuda_dev, dtype=torch.bfloat16)
    wp = pack_fwd(w)
    d = dict(_geo(N, H), C1=Cin, src1=ptr(x), wgt=ptr(wp), bias=ptr(b), Cout=Cout, dst1=ptr(y))
    rows = [C().conv_stat_tiles(dict(d, stats=1, win_bm2=m))[0] for m in (0, 3)]
    assert rows[0] == rows[1] == N * H * H // 256
    st = torch.empty(rows[0] * 2 * Cout, device=cuda_dev)
    _ab(dict(d, stats=ptr(st)), [y, st], halves=False)


def test_win512_keeps_256_in_3d(cuda_dev):
    torch.manual_seed(188)
    N, D, H, Cin, Cout = 1, 2, 32, 32, 64
    x = torch.randn(N, D, H, H, Cin, device=cuda_dev).bfloat16()
    w = (torch.randn(3, 3, 3, Cin, Cout, device=cuda_dev) * 0.05).bfloat16()
    b = torch.randn(Cout, device=cuda_dev) * 0.1
    y = torch.empty(N, D, H, H, Cout, device=cuda_dev, dtype=torch.bfloat16)
    wp = pad64(w.permute(4, 0, 1, 2, 3).reshape(Cout, -1))
    d = dict(N=N, OD=D, OH=H, OW=H, ID=D, IH=H, IW=H, KD=3, KH=3, KW=3, pad=1, C1=Cin, src1=ptr(x), wgt=ptr(wp),
             bias=ptr(b), Cout=Cout, relu=1, dst1=ptr(y))
    _ab(d, [y], halves=False)


# ------------------------------------------------------------------------ whole step
def test_win512_step_is_bit_identical(cuda_dev, monkeypatch):
    """One training step of the 128^2 model with win_bm2 = 0 against 3: loss sums,
    probabilities, the first layer's activation gradient and every parameter gradient."""
    from test_gpu_model import _setup
    outs = []
    for v in ("0", "3"):
        monkeypatch.setenv("UNET_ENGINE", "win_bm2=" + v)
        spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, batch_size=4, img_size=128, in_channels=4)
        e = nb.engine
        assert e.opts["win_bm2"] == int(v)
        nb.fwd_bwd(x, y, seed=31)
        torch.cuda.synchronize()
        outs.append((nb.sums().cpu(), e.prob.clone(), e.bufs["d:conv1a"].clone(),
                     {k: fn.view(fn.grad, k).clone() for k, *_ in fn.entries}))
    (s0, p0, d0, g0), (s1, p1, d1, g1) = outs
    assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(d0, d1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k

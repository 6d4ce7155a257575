"""Pipelined window loop of the fused data + weight gradient (conv_dw.hip PIPE, fw_pipe=1)
against the serial loop (fw_pipe=0) and an fp32 torch reference, on window ranges small
enough to hit every prefetch case: one window, only non-carried windows, carried and
non-carried alternating, ranges that cross image boundaries, empty and one-window
workgroups, long carried runs.  Operands and MFMA order are the same in both loops, so the
outputs must be bit-identical; each loop is also held to the reference on its own."""

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import C, nchw, nhwc, pack_dgrad, ptr, rel_err, stream

pytestmark = pytest.mark.gpu

W = 128
SPLIT_LO, ROWS_ABOVE = 3, 2
# N, H, nsplit
SHAPES = [(1, 2, 1), (3, 2, 1), (3, 4, 1), (5, 6, 4), (2, 4, 7), (2, 128, 7)]
# dY source: plain tensor (XF 0) / formed on load from the head (XF 4) with BCE weight 0 and 0.5
SOURCES = [("plain", 0.0), ("head", 0.0), ("head", 0.5)]


def _bits(act):
    v = (act.float() > 0).reshape(-1, 8).to(torch.int32)
    return (v << torch.arange(8, device=act.device, dtype=torch.int32)).sum(1).to(torch.uint8)


def _head(y, hw, t, gsc, bce):
    """Probability, loss sums and the materialised dY of head input y, as
    test_gpu_conv_dw.py::test_fused_dgrad_wgrad_head_on_load forms them (head_fwd, head_bwd)."""
    P = t.numel()
    hb = torch.randn(1, device=y.device)
    prob = torch.empty(P, device=y.device)
    nb = C().head_blocks(P)
    part = torch.empty(nb * 33 + 4 * nb, device=y.device)
    sums = torch.empty(4, device=y.device)
    C().generic("head_fwd", [ptr(y), ptr(hw), ptr(hb), ptr(t), ptr(prob), ptr(part), ptr(sums)], [P, 32], [], stream())
    dy = torch.empty_like(y)
    ow, ob = torch.empty(32, device=y.device), torch.empty(1, device=y.device)
    C().generic("head_bwd", [ptr(y), ptr(hw), ptr(prob), ptr(t), ptr(sums), ptr(dy), ptr(part), ptr(ow), ptr(ob),
                             ptr(gsc)], [P, 32], [1.0 / P, bce, 1.0], stream())
    torch.cuda.synchronize()
    return prob, sums, dy


@pytest.mark.parametrize("src,bce", SOURCES)
@pytest.mark.parametrize("N,H,nsplit", SHAPES)
def test_pipelined_loop_matches_serial_loop_and_reference(cuda_dev, N, H, nsplit, src, bce):
    torch.manual_seed(1000 * N + 10 * H + nsplit)
    dev = cuda_dev
    P = N * H * W
    x = F.relu(torch.randn(N, H, W, 32, device=dev)).bfloat16()          # the conv's forward input
    act = F.relu(torch.randn(N, H, W, 32, device=dev)).bfloat16()        # ReLU output the gradient is masked by
    w = (torch.randn(3, 3, 32, 32, device=dev) * 0.1).bfloat16()
    wp = pack_dgrad(w)                       # (kept alive: the launches below read it)
    mbits = _bits(act)
    base = dict(N=N, OH=H, OW=W, IH=H, IW=W, KH=3, KW=3, pad=1, C1=32, wgt=ptr(wp), Cout=32, relu=0,
                mask1=ptr(mbits), mask_bits=1, fw_x=ptr(x), fw_Cx=32, fw_nsplit=nsplit, fw_split_lo=SPLIT_LO)
    if src == "plain":
        dy = torch.randn(N, H, W, 32, device=dev).bfloat16()
        base.update(src1=ptr(dy))
    else:
        y = F.relu(torch.randn(N, H, W, 32, device=dev)).bfloat16()      # the head input
        ybits = _bits(y)
        hw = 0.3 * torch.randn(32, device=dev)
        t = (torch.rand(P, device=dev) > 0.7).bfloat16()
        gsc = torch.full((1,), 2.0, device=dev)
        prob, sums, dy = _head(y, hw, t, gsc, bce)
        base.update(src1=ptr(x), hg_prob=ptr(prob), hg_t=ptr(t), hg_sums=ptr(sums), hg_w=ptr(hw),    # (src1 unused)
                    hg_bits=ptr(ybits), hg_gscale=ptr(gsc), hg_inv_total=1.0 / P, hg_bce_w=bce)

    # fp32 reference from the same 16-bit inputs
    xr = nchw(x.float()).requires_grad_(True)
    wr = w.float().permute(3, 2, 0, 1).clone().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(xr, wr, padding=1), (xr, wr), nchw(dy.float()))
    ref_dx = nhwc(gx) * (act.float() > 0)
    ref_w = gw.permute(2, 3, 1, 0).reshape(9, 32, 32)                     # [tap][ci][co]
    ref_b = dy.float().sum((0, 1, 2))

    nwin = N * H // 2
    empty = [k for k in range(nsplit) if k * nwin // nsplit == (k + 1) * nwin // nsplit]
    rows = SPLIT_LO + nsplit + ROWS_ABOVE
    outs = []
    for pipe in (0, 1, 1):
        dx = torch.full((N, H, W, 32), 7.0, device=dev, dtype=torch.bfloat16)
        slab = torch.full((rows, 9, 32, 32), float("nan"), device=dev)
        bslab = torch.full((rows, 32), float("nan"), device=dev)
        d = dict(base, dst1=ptr(dx), fw_slab=ptr(slab), fw_bias_slab=ptr(bslab), fw_pipe=pipe)
        assert C().conv_fwd_grid(d) == nsplit
        C().conv_fwd(d, stream())
        outs.append((dx, slab, bslab))
    torch.cuda.synchronize()

    for arm, (dx, slab, bslab) in zip(("serial", "pipelined", "pipelined again"), outs):
        lo, hi = SPLIT_LO, SPLIT_LO + nsplit
        # rows outside the launch's range are untouched, empty workgroups write zeros
        assert torch.isnan(slab[:lo]).all() and torch.isnan(bslab[:lo]).all(), arm
        assert torch.isnan(slab[hi:]).all() and torch.isnan(bslab[hi:]).all(), arm
        for k in empty:
            assert (slab[lo + k] == 0).all() and (bslab[lo + k] == 0).all(), (arm, k)
        e_w = rel_err(slab[lo:hi].double().sum(0).float(), ref_w)
        e_b = rel_err(bslab[lo:hi].double().sum(0).float(), ref_b)
        e_x = ((dx.float() - ref_dx).abs().max() / ref_dx.abs().max()).item()
        print("%s: slab %.3g bias %.3g dx %.3g" % (arm, e_w, e_b, e_x))
        assert e_w < 1e-4, (arm, e_w)
        assert e_b < 1e-4, (arm, e_b)
        assert e_x < 2.0 ** -8, (arm, e_x)
    for arm, other in (("pipelined", outs[1]), ("pipelined again", outs[2])):
        for name, a, b in zip(("dst1", "fw_slab", "fw_bias_slab"), outs[0], other):
            assert torch.equal(a[SPLIT_LO:SPLIT_LO + nsplit] if name != "dst1" else a,
                               b[SPLIT_LO:SPLIT_LO + nsplit] if name != "dst1" else b), (arm, name)


def test_pipelined_loop_step_is_bit_identical(cuda_dev, monkeypatch):
    """One training step with dw_pipe=0 against dw_pipe=1: loss sums, probabilities, the
    first layer's activation gradient and every parameter gradient (conv1b's and conv9b's,
    which the fused kernel produces, included) are bit-identical."""
    from test_gpu_model import _setup
    outs = []
    for v in ("0", "1"):
        monkeypatch.setenv("UNET_ENGINE", "dw_pipe=" + v)
        spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, batch_size=4, img_size=128, in_channels=4)
        e = nb.engine
        assert sorted(e.fusions.get("dw_fused", [])) == ["conv1b", "conv9b"]
        nb.fwd_bwd(x, y, seed=31)
        torch.cuda.synchronize()
        outs.append((nb.sums().cpu(), e.prob.clone(), e.bufs["d:conv1a"].clone(),
                     {k: fn.view(fn.grad, k).clone() for k, *_ in fn.entries}))
    (s0, p0, d0, g0), (s1, p1, d1, g1) = outs
    assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(d0, d1)
    assert any(k.startswith("conv1b/") for k in g0) and any(k.startswith("conv9b/") for k in g0)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k

"""Training-time augmentation on the GPU: the augmenting batch gather
(csrc/kernels/gather.h, ops gather_batch_aug / f32_gather_batch_aug) against
data/augment.py's apply_torch on the plain gather's output -- bit for bit, the geometric
transform is a permutation -- the intensity affine against float64 within one rounding to
the storage type, and the executors' load_indexed(aug=...) against pre-augmented tensors.
"""
import functools

import pytest
import torch

from unet_distributed_amd.data import augment as A

pytestmark = pytest.mark.gpu

PAD = 4096              # guard elements on each side of an output
NALL = 11               # samples of the resident dataset
# name: (torch dtype, op, dtype id, unit roundoff of one rounding to the type)
TYPES = {"bf16": (torch.bfloat16, "gather_batch_aug", 0, 2.0 ** -8),
         "fp16": (torch.float16, "gather_batch_aug", 1, 2.0 ** -11),
         "fp32": (torch.float32, "f32_gather_batch_aug", 0, 2.0 ** -24)}
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr()) if t is not None else 0


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """An output of `n` elements in the middle of a NaN-filled buffer: after the launch the
    payload is finite and the guard regions are still NaN."""

    def __init__(self, n, dtype, dev):
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=dev)
        self.out = self.buf[PAD:PAD + n]

    def check(self):
        assert torch.isfinite(self.out.float()).all()
        assert torch.isnan(self.buf[:PAD].float()).all()
        assert torch.isnan(self.buf[PAD + self.out.numel():].float()).all()


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


@functools.lru_cache(maxsize=None)
def dataset(D, H, cin, K):
    """The resident fp32 dataset of one shape, shared by the tests that read it."""
    g = torch.Generator().manual_seed(1000 * D + 10 * H + cin + K)
    shape = (NALL, H, H) if D == 1 else (NALL, D, H, H)
    x = torch.randn(shape + (cin,), generator=g)
    y = (torch.rand(shape + (K,), generator=g) > 0.6).float()
    return x.cuda(), y.cuda()


def batch_idx(B, dev):
    """Unsorted sample indices out of NALL with one repeat."""
    idx = [9, 2, 7, 2, 10, 0, 5, 3, 8, 1, 6, 4, 9, 7, 0, 10][:B]
    return torch.tensor(idx, dtype=torch.int64, device=dev)


def plain_gather(x_all, y_all, idx, tname, cpad):
    """The batch as the un-augmented path leaves it: the gather_batch kernel for the 16-bit
    types, index_select for fp32 (padded with zero channels when cpad > Cin)."""
    dt, _, dt_id, _ = TYPES[tname]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    P = x_all[0].numel() // cin
    if tname == "fp32":
        xs = x_all.index_select(0, idx)
        xb = xs.new_zeros(xs.shape[:-1] + (cpad,))
        xb[..., :cin] = xs
        return xb, y_all.index_select(0, idx)
    xb = torch.empty((B,) + tuple(x_all.shape[1:-1]) + (cpad,), dtype=dt, device=x_all.device)
    tb = torch.empty((B,) + tuple(y_all.shape[1:]), dtype=dt, device=x_all.device)
    C().generic("gather_batch", [ptr(x_all), ptr(y_all), ptr(idx), ptr(xb), ptr(tb)], [B, P, cin, cpad, K], [],
                stream(), dt_id)
    return xb, tb


def aug_gather(x_all, y_all, idx, code, affine, tname, cpad):
    """gather_batch_aug / f32_gather_batch_aug into guarded buffers."""
    dt, op, dt_id, _ = TYPES[tname]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    D = x_all.shape[1] if x_all.dim() == 5 else 1
    H, W = x_all.shape[-3], x_all.shape[-2]
    xb = Guarded(B * D * H * W * cpad, dt, x_all.device)
    tb = Guarded(B * D * H * W * K, dt, x_all.device)
    C().generic(op, [ptr(x_all), ptr(y_all), ptr(idx), ptr(code), ptr(affine), ptr(xb.out), ptr(tb.out)],
                [B, D, H, W, cin, cpad, K], [], stream(), dt_id)
    torch.cuda.synchronize()
    xb.check()
    tb.check()
    return xb.out.view((B,) + tuple(x_all.shape[1:-1]) + (cpad,)), tb.out.view((B,) + tuple(y_all.shape[1:]))


def cpad_of(tname, cin):
    return cin if tname == "fp32" else (4 if cin <= 4 else 8 if cin <= 8 else cin)


def check_geometric(dev, tname, D, H, cin, K, B, cpad=None):
    cpad = cpad or cpad_of(tname, cin)
    x_all, y_all = dataset(D, H, cin, K)
    idx = batch_idx(B, dev)
    ncode = 8 if D == 1 else 16
    code = torch.tensor([(3 * i + 5) % ncode for i in range(B)], dtype=torch.int32)     # every code, shuffled
    assert sorted(code.tolist()) == sorted(list(range(ncode)) * (B // ncode))
    xp, tp = plain_gather(x_all, y_all, idx, tname, cpad)
    wx, wt = A.apply_torch(xp, tp, code)
    gx, gt = aug_gather(x_all, y_all, idx, code.to(dev), None, tname, cpad)
    assert torch.equal(bits(gx), bits(wx)), (tname, D, H, cin, cpad, K, "image")
    assert torch.equal(bits(gt), bits(wt)), (tname, D, H, cin, cpad, K, "target")
    if cpad > cin:
        assert (gx[..., cin:] == 0).all()
    return gx, gt


@pytest.mark.parametrize("H", [16, 48, 128])
@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_geometric_2d_is_a_permutation_of_the_plain_gather(cuda_dev, tname, H):
    """H = 16: smaller than the 32-pixel tile (and the 32-wide strip); 48: one and a half tiles
    (three quarters of a 64-wide strip); 128: 16 whole tiles (8-row strips of whole rows)."""
    for cin in (1, 4):
        for K in (1, 3):
            check_geometric(cuda_dev, tname, 1, H, cin, K, 8)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_geometric_3d_all_sixteen_codes(cuda_dev, tname):
    check_geometric(cuda_dev, tname, 16, 16, 4, 2, 16)


@pytest.mark.parametrize("tname,cin,cpad", [("bf16", 8, 8), ("fp16", 5, 8), ("bf16", 32, 32), ("fp32", 8, 8),
                                            ("fp32", 5, 5), ("fp32", 3, 4)])
def test_kernel_geometric_other_channel_counts(cuda_dev, tname, cin, cpad):
    """The 8-channel tiles (16- and 32-byte pixels), their scalar-load form (Cin < Cpad) and
    the per-pixel kernel of every other Cpad."""
    check_geometric(cuda_dev, tname, 1, 48, cin, 2, 8, cpad)


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_kernel_geometric_rows_wider_than_a_strip(cuda_dev, tname):
    """W = 160: the codes without T work on 128-pixel strips, so a row is a strip and a 32-pixel
    rest, and the strip tiling has more workgroups per image (40) than the 32 x 32 tiling (25)."""
    check_geometric(cuda_dev, tname, 1, 160, 4, 1, 8)


def test_code_bits_outside_the_dims_are_ignored(cuda_dev):
    """2D: bit 3 (flip D) and anything above are masked off by the kernel."""
    x_all, y_all = dataset(1, 48, 4, 1)
    idx = batch_idx(8, cuda_dev)
    code = torch.arange(8, dtype=torch.int32, device=cuda_dev)
    a = aug_gather(x_all, y_all, idx, code, None, "bf16", 4)
    b = aug_gather(x_all, y_all, idx, code + 8 + 64, None, "bf16", 4)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_intensity_within_one_rounding(cuda_dev, tname):
    """|out - r| <= 2 u |r| + 2^-22 (|scale x| + |shift|) + 2^-24 with r = scale x + shift in
    float64: one rounding to the storage type (unit roundoff u) with a factor-2 margin, plus
    the fp32 evaluation of the fma."""
    dev, H, B = cuda_dev, 48, 8
    u = TYPES[tname][3]
    worst = 0.0
    for D, cin, K in ((1, 1, 1), (1, 4, 3), (1, 4, 1), (1, 1, 3), (16, 4, 2)):
        Hh, Bb = (H, B) if D == 1 else (16, 16)
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(D, Hh, cin, K)
        idx = batch_idx(Bb, dev)
        ncode = 8 if D == 1 else 16
        code = torch.tensor([(3 * i + 5) % ncode for i in range(Bb)], dtype=torch.int32)
        g = torch.Generator().manual_seed(cin + K)
        a = 0.25
        aff = torch.stack([1 - a + 2 * a * torch.rand(Bb, cin, generator=g),
                           -a + 2 * a * torch.rand(Bb, cin, generator=g)], dim=-1).contiguous()
        gx, gt = aug_gather(x_all, y_all, idx, code.to(dev), aff.to(dev), tname, cpad)
        _, t0 = aug_gather(x_all, y_all, idx, code.to(dev), None, tname, cpad)
        assert torch.equal(bits(gt), bits(t0))                  # the target: geometry only
        xg, _ = A.apply_torch(x_all.index_select(0, idx), y_all.index_select(0, idx), code)
        sh = (Bb,) + (1,) * (xg.dim() - 2) + (cin,)
        s, t = aff[..., 0].to(dev).double().view(sh), aff[..., 1].to(dev).double().view(sh)
        r = s * xg.double() + t
        bound = 2 * u * r.abs() + 2.0 ** -22 * ((s * xg.double()).abs() + t.abs()) + 2.0 ** -24
        err = (gx[..., :cin].double() - r).abs()
        worst = max(worst, float((err / bound).max()))
        print("intensity", tname, (D, cin, K), "max err / bound", float((err / bound).max()))
        assert (err <= bound).all(), (tname, D, cin, K)
        if cpad > cin:
            assert (gx[..., cin:] == 0).all()                   # pad channels stay zero
    assert worst > 0                                            # (the affine was applied at all)


# ------------------------------------------------------------------ executors
def _backend(dev, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(batch_size=4, img_size=32, in_channels=4, synthetic=True, no_checkpoint=True, **kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    return cfg, flat, NativeBackend(spec, flat, cfg, dev, 4)


def _resident(dev, cfg, aug):
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.data.loader import ResidentBatch
    x, y = synthetic_brats(NALL, cfg.img_size, cfg.in_channels, cfg.dims, seed=5, out_channels=cfg.out_channels)
    idx = torch.tensor([1, 4, 4, 9], dtype=torch.int64, device=dev)
    return ResidentBatch(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), idx, aug)


@pytest.mark.parametrize("kw", [dict(out_channels=1), dict(out_channels=3), dict(out_channels=1, dtype="fp32")],
                         ids=["bf16-K1", "bf16-K3", "fp32-K1"])
def test_executor_step_on_an_augmented_resident_batch(cuda_dev, kw):
    """fwd_bwd on a ResidentBatch carrying geometric parameters == fwd_bwd on the tensors
    augmented beforehand, at the same dropout seed: the same loss sums and gradient bits."""
    cfg, flat, be = _backend(cuda_dev, **kw)
    code = torch.tensor([5, 2, 7, 0], dtype=torch.int32, device=cuda_dev)
    rb = _resident(cuda_dev, cfg, (code, None))
    be.fwd_bwd(rb, None, seed=77)
    torch.cuda.synchronize()
    s1, g1 = be.sums().clone(), flat.grad.clone()
    x, y = rb.tensors()
    px, _ = _resident(cuda_dev, cfg, None).tensors()
    assert not torch.equal(x, px) and torch.equal(x[3], px[3])          # (augmented; code 0 is the identity)
    be.fwd_bwd(x.contiguous(), y.contiguous(), seed=77)
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all() and g1.abs().sum() > 0
    assert torch.equal(bits(s1), bits(be.sums())) and torch.equal(bits(g1), bits(flat.grad))


def test_resident_feeder_uploads_the_parameters_with_the_indices(cuda_dev):
    """DeviceFeeder on resident data: the parameters are drawn for the sorted indices, reach the
    device unchanged in the one upload, and the lazy batch, its tensors and the non-lazy batch
    are the same augmented batch; an executor takes the lazy batch as it comes."""
    from unet_distributed_amd.data.loader import DeviceFeeder
    cfg, flat, be = _backend(cuda_dev, out_channels=1)
    rb0 = _resident(cuda_dev, cfg, None)
    f = DeviceFeeder(rb0.x_all.cpu().numpy(), rb0.y_all.cpu().numpy(), 4, cuda_dev, mode="on")
    assert f.resident
    idx = [9, 1, 4, 4]
    aug = lambda si: A.draw(3, 5, si, "flip,rot90,intensity", 4, 2, 0.2)  # noqa: E731
    rb, none = f.get(idx, lazy=True, aug=aug)
    code, aff = A.draw(3, 5, sorted(idx), "flip,rot90,intensity", 4, 2, 0.2)
    assert none is None and rb.idx.tolist() == sorted(idx) and rb.idx.dtype == torch.int64
    assert rb.aug[0].dtype == torch.int32 and rb.aug[0].cpu().tolist() == code.tolist()
    assert rb.aug[1].dtype == torch.float32 and rb.aug[1].is_contiguous()
    assert torch.equal(rb.aug[1].cpu(), torch.from_numpy(aff))
    x, y = f.get(idx, aug=aug)
    tx, ty = rb.tensors()
    wx, wy = A.apply_torch(rb0.x_all[sorted(idx)], rb0.y_all[sorted(idx)], code, aff)
    assert torch.equal(x, wx) and torch.equal(y, wy) and torch.equal(tx, wx) and torch.equal(ty, wy)
    be.engine.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=rb.aug)
    torch.cuda.synchronize()
    got = be.engine.bufs["x"].view(wx.shape).float()
    assert (got - wx).abs().max() <= 2.0 ** -8 * wx.abs().max()         # (bf16 of the same pixels)
    assert torch.equal(be.engine.target.view(wy.shape).float(), wy)


@pytest.mark.parametrize("kw", [dict(out_channels=3), dict(out_channels=1, dtype="fp16"),
                                dict(out_channels=1, dtype="fp32")], ids=["bf16-K3", "fp16-K1", "fp32-K1"])
def test_load_indexed_without_aug_is_the_plain_gather(cuda_dev, kw):
    cfg, flat, be = _backend(cuda_dev, **kw)
    e = be.engine
    rb = _resident(cuda_dev, cfg, None)
    tname = cfg.dtype
    cpad = cpad_of(tname, 4)
    wx, wt = plain_gather(rb.x_all, rb.y_all, rb.idx, tname, cpad)
    # the plain call, then the identity code through the new op: the same buffers both times
    for aug in (None, (torch.zeros(4, dtype=torch.int32, device=cuda_dev), None)):
        e.bufs["x"].fill_(7)
        e.target.fill_(7)
        if aug is None:
            e.load_indexed(rb.x_all, rb.y_all, rb.idx)
        else:
            e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=aug)
        torch.cuda.synchronize()
        assert torch.equal(bits(e.bufs["x"].view(-1)), bits(wx.view(-1)))
        assert torch.equal(bits(e.target.view(-1)), bits(wt.view(-1)))

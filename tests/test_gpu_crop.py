"""Patch-sampled training on the GPU: the cropping batch gather (csrc/kernels/gather.h,
ops gather_batch_crop / f32_gather_batch_crop) against the definition in plain torch --
apply_torch(crop_torch(index_select)) cast to the storage type, bit for bit: cropping and the
geometric transform only move pixels -- the intensity affine against float64 within one
rounding, origins outside the sample against the oracle at the clamped origin, the executors'
load_indexed(crop=...) against pre-cropped tensors, the feeder's upload, and one CLI run.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from unet_distributed_amd.data import augment as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 4096              # guard elements on each side of an output
NALL = 5                # samples of the resident dataset
# name: (torch dtype, crop op, aug op, dtype id, unit roundoff of one rounding to the type)
TYPES = {"bf16": (torch.bfloat16, "gather_batch_crop", "gather_batch_aug", 0, 2.0 ** -8),
         "fp16": (torch.float16, "gather_batch_crop", "gather_batch_aug", 1, 2.0 ** -11),
         "fp32": (torch.float32, "f32_gather_batch_crop", "f32_gather_batch_aug", 0, 2.0 ** -24)}
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
def dataset(stored, cin, K):
    """The resident fp32 dataset of one stored shape ((Hs, Ws) or (Ds, Hs, Ws)), shared by the
    tests that read it and never written."""
    g = torch.Generator().manual_seed(sum(stored) * 100 + 10 * cin + K)
    x = torch.randn((NALL,) + tuple(stored) + (cin,), generator=g)
    y = (torch.rand((NALL,) + tuple(stored) + (K,), generator=g) > 0.6).float()
    return x.cuda(), y.cuda()


def batch_idx(B, dev):
    """Unsorted sample indices out of NALL with repeats."""
    idx = [3, 2, 4, 2, 0, 1, 3, 4, 1, 0, 2, 4, 3, 1, 0, 2][:B]
    return torch.tensor(idx, dtype=torch.int64, device=dev)


def origins(B, stored3, patch3):
    """int32 [B][3]: 0, the maximum, odd values and mixtures, all inside [0, S - T]."""
    mx = [s - t for s, t in zip(stored3, patch3)]
    rows = [(0, 0, 0), tuple(mx), (1, 1, 3), (mx[0], 0, mx[2]), (0, mx[1], 0), (3, 5, 7), (mx[0] - 1, mx[1] - 1, 1),
            (1, mx[1], mx[2] - 1)]
    rows = [tuple(min(max(v, 0), m) for v, m in zip(r, mx)) for r in rows]
    return torch.tensor([rows[i % len(rows)] for i in range(B)], dtype=torch.int32)


def dims3(v):
    return (1,) + tuple(v) if len(v) == 2 else tuple(v)


def crop_gather(x_all, y_all, idx, origin, code, affine, tname, cpad, patch):
    """gather_batch_crop / f32_gather_batch_crop into guarded buffers; patch (H, W) or (D, H, W)."""
    dt, op, _, dt_id, _ = TYPES[tname]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    Ds, Hs, Ws = dims3(x_all.shape[1:-1])
    D, H, W = dims3(patch)
    xb = Guarded(B * D * H * W * cpad, dt, x_all.device)
    tb = Guarded(B * D * H * W * K, dt, x_all.device)
    C().generic(op, [ptr(x_all), ptr(y_all), ptr(idx), ptr(origin), ptr(code), ptr(affine), ptr(xb.out), ptr(tb.out)],
                [B, Ds, Hs, Ws, D, H, W, cin, cpad, K], [], stream(), dt_id)
    torch.cuda.synchronize()
    xb.check()
    tb.check()
    return xb.out.view((B,) + tuple(patch) + (cpad,)), tb.out.view((B,) + tuple(patch) + (K,))


def oracle(x_all, y_all, idx, origin, code, affine, tname, cpad, patch):
    """apply_torch(crop_torch(plain index_select)) cast to the type, zero pad channels."""
    dt = TYPES[tname][0]
    x, y = A.crop_torch(x_all.index_select(0, idx), y_all.index_select(0, idx), origin, dims3(patch))
    x, y = A.apply_torch(x, y, code, affine)
    xb = torch.zeros(x.shape[:-1] + (cpad,), dtype=dt, device=x.device)
    xb[..., :x.shape[-1]] = x.to(dt)
    return xb, y.to(dt)


def cpad_of(tname, cin):
    return cin if tname == "fp32" else (4 if cin <= 4 else 8 if cin <= 8 else cin)


def check_geometric(dev, tname, stored, patch, cin, K, B, cpad=None):
    cpad = cpad or cpad_of(tname, cin)
    x_all, y_all = dataset(tuple(stored), cin, K)
    idx = batch_idx(B, dev)
    ncode = 8 if len(stored) == 2 else 16
    code = torch.tensor([(3 * i + 5) % ncode for i in range(B)], dtype=torch.int32)     # every code, shuffled
    assert sorted(code.tolist()) == sorted(list(range(ncode)) * (B // ncode))
    org = origins(B, dims3(stored), dims3(patch))
    wx, wt = oracle(x_all, y_all, idx, org, code, None, tname, cpad, patch)
    gx, gt = crop_gather(x_all, y_all, idx, org.to(dev), code.to(dev), None, tname, cpad, patch)
    assert torch.equal(bits(gx), bits(wx)), (tname, stored, patch, cin, cpad, K, "image")
    assert torch.equal(bits(gt), bits(wt)), (tname, stored, patch, cin, cpad, K, "target")
    if cpad > cin:
        assert (gx[..., cin:] == 0).all()
    # two runs give the same bits
    hx, ht = crop_gather(x_all, y_all, idx, org.to(dev), code.to(dev), None, tname, cpad, patch)
    assert torch.equal(bits(gx), bits(hx)) and torch.equal(bits(gt), bits(ht))
    return gx, gt


@pytest.mark.parametrize("T", [16, 32, 40])
@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_2d_patches_of_a_non_square_sample(cuda_dev, tname, T):
    """Stored 40 x 56 (not square, no multiple of 32): patches smaller than a tile, of one tile,
    and of a whole stored axis (40: the h origin can only be 0)."""
    for cin in (1, 4):
        for K in (1, 3):
            check_geometric(cuda_dev, tname, (40, 56), (T, T), cin, K, 8)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_2d_whole_row_strips_at_a_pitch(cuda_dev, tname):
    """Patch 128 of 136 x 200: the strips are whole patch rows, 200 pixels apart in the source."""
    check_geometric(cuda_dev, tname, (136, 200), (128, 128), 4, 1, 8)


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_kernel_2d_rows_wider_than_a_strip(cuda_dev, tname):
    """Patch 160 of 176 x 200: a row is a 128-pixel strip and a 32-pixel rest."""
    check_geometric(cuda_dev, tname, (176, 200), (160, 160), 4, 1, 8)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_3d_all_sixteen_codes(cuda_dev, tname):
    check_geometric(cuda_dev, tname, (20, 24, 28), (16, 16, 16), 4, 2, 16)


@pytest.mark.parametrize("tname,cin,cpad", [("bf16", 8, 8), ("fp16", 5, 8), ("bf16", 32, 32), ("fp32", 8, 8),
                                            ("fp32", 5, 8), ("fp32", 32, 32), ("fp32", 3, 4)])
def test_kernel_other_channel_counts(cuda_dev, tname, cin, cpad):
    """The 8-channel tiles, their scalar-load form (Cin < Cpad) and the per-pixel kernel."""
    check_geometric(cuda_dev, tname, (40, 56), (32, 32), cin, 2, 8, cpad)


@pytest.mark.parametrize("tname", list(TYPES))
def test_null_code_is_the_identity_code(cuda_dev, tname):
    dev = cuda_dev
    for stored, patch, cin in (((40, 56), (32, 32), 4), ((40, 56), (16, 16), 32), ((20, 24, 28), (16, 16, 16), 4)):
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, 2)
        B = 8
        idx, org = batch_idx(B, dev), origins(B, dims3(stored), dims3(patch)).to(dev)
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        a = crop_gather(x_all, y_all, idx, org, None, None, tname, cpad, patch)
        b = crop_gather(x_all, y_all, idx, org, zero, None, tname, cpad, patch)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
        w = oracle(x_all, y_all, idx, org, zero, None, tname, cpad, patch)
        assert torch.equal(bits(a[0]), bits(w[0])) and torch.equal(bits(a[1]), bits(w[1]))


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_intensity_within_one_rounding(cuda_dev, tname):
    """|out - r| <= 2 u |r| + 2^-22 (|scale x| + |shift|) + 2^-24 with r = scale x + shift in
    float64: one rounding to the storage type (unit roundoff u) with a factor-2 margin, plus
    the fp32 evaluation of the fma -- the bound of the un-cropped gather's test."""
    dev = cuda_dev
    u = TYPES[tname][4]
    worst = 0.0
    for stored, patch, cin, K, B in (((40, 56), (32, 32), 1, 1, 8), ((40, 56), (32, 32), 4, 3, 8),
                                     ((40, 56), (16, 16), 4, 1, 8), ((20, 24, 28), (16, 16, 16), 4, 2, 16)):
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx = batch_idx(B, dev)
        ncode = 8 if len(stored) == 2 else 16
        code = torch.tensor([(3 * i + 5) % ncode for i in range(B)], dtype=torch.int32)
        org = origins(B, dims3(stored), dims3(patch))
        g = torch.Generator().manual_seed(cin + K)
        a = 0.25
        aff = torch.stack([1 - a + 2 * a * torch.rand(B, cin, generator=g),
                           -a + 2 * a * torch.rand(B, cin, generator=g)], dim=-1).contiguous()
        gx, gt = crop_gather(x_all, y_all, idx, org.to(dev), code.to(dev), aff.to(dev), tname, cpad, patch)
        _, t0 = crop_gather(x_all, y_all, idx, org.to(dev), code.to(dev), None, tname, cpad, patch)
        assert torch.equal(bits(gt), bits(t0))                  # the target: geometry only
        xg, _ = A.apply_torch(*A.crop_torch(x_all.index_select(0, idx), y_all.index_select(0, idx), org,
                                            dims3(patch)), code)
        sh = (B,) + (1,) * (xg.dim() - 2) + (cin,)
        s, t = aff[..., 0].to(dev).double().view(sh), aff[..., 1].to(dev).double().view(sh)
        r = s * xg.double() + t
        bound = 2 * u * r.abs() + 2.0 ** -22 * ((s * xg.double()).abs() + t.abs()) + 2.0 ** -24
        err = (gx[..., :cin].double() - r).abs()
        worst = max(worst, float((err / bound).max()))
        print("intensity", tname, (stored, patch, cin, K), "max err / bound", float((err / bound).max()))
        assert (err <= bound).all(), (tname, stored, cin, K)
        if cpad > cin:
            assert (gx[..., cin:] == 0).all()
    assert worst > 0


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_origins_outside_the_sample_are_clamped(cuda_dev, tname):
    """Negative and too large origins (device data no launch can validate) read the patch at the
    origin clamped into [0, S - T]: tiled and per-pixel kernels, 2D and 3D."""
    dev = cuda_dev
    for stored, patch, cin in (((40, 56), (32, 32), 4), ((40, 56), (32, 32), 32), ((20, 24, 28), (16, 16, 16), 4)):
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, 2)
        B = 8
        S, T = dims3(stored), dims3(patch)
        wild = torch.tensor([(-1, -1, -1), (0, -7, 1000), (5000, 9, -3), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1),
                             (-2 ** 31, -2 ** 31, -2 ** 31), (1, S[1] - T[1] + 1, 3), (0, 2, S[2] - T[2] + 1),
                             (S[0] - T[0] + 1, 0, 0)], dtype=torch.int32)
        mx = torch.tensor([s - t for s, t in zip(S, T)], dtype=torch.int32)
        clamped = torch.minimum(torch.clamp(wild, min=0), mx[None, :])
        idx = batch_idx(B, dev)
        code = torch.arange(B, dtype=torch.int32)
        g = crop_gather(x_all, y_all, idx, wild.to(dev), code.to(dev), None, tname, cpad, patch)
        w = oracle(x_all, y_all, idx, clamped, code, None, tname, cpad, patch)
        assert torch.equal(bits(g[0]), bits(w[0])) and torch.equal(bits(g[1]), bits(w[1])), (tname, stored, cin)


@pytest.mark.parametrize("tname", list(TYPES))
def test_patch_of_the_stored_size_is_the_augmenting_gather(cuda_dev, tname):
    """Stored size == patch size, origin 0: bit-identical to gather_batch_aug, geometry and affine."""
    dev = cuda_dev
    dt, _, aug_op, dt_id, _ = TYPES[tname]
    for stored, cin, K, B in (((48, 48), 4, 3, 8), ((48, 48), 1, 1, 8), ((16, 16, 16), 4, 2, 16)):
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx = batch_idx(B, dev)
        ncode = 8 if len(stored) == 2 else 16
        code = torch.tensor([(3 * i + 5) % ncode for i in range(B)], dtype=torch.int32, device=dev)
        gen = torch.Generator().manual_seed(7)
        aff = torch.stack([0.8 + 0.4 * torch.rand(B, cin, generator=gen),
                           -0.2 + 0.4 * torch.rand(B, cin, generator=gen)], dim=-1).contiguous().to(dev)
        D, H, W = dims3(stored)
        for af in (None, aff):
            xb = torch.empty(B * D * H * W * cpad, dtype=dt, device=dev)
            tb = torch.empty(B * D * H * W * K, dtype=dt, device=dev)
            C().generic(aug_op, [ptr(x_all), ptr(y_all), ptr(idx), ptr(code), ptr(af), ptr(xb), ptr(tb)],
                        [B, D, H, W, cin, cpad, K], [], stream(), dt_id)
            org = torch.zeros(B, 3, dtype=torch.int32, device=dev)
            gx, gt = crop_gather(x_all, y_all, idx, org, code, af, tname, cpad, stored)
            assert torch.equal(bits(gx.reshape(-1)), bits(xb)) and torch.equal(bits(gt.reshape(-1)), bits(tb))


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


def _resident(dev, cfg, aug, crop, stored=48):
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.data.loader import ResidentBatch
    x, y = synthetic_brats(NALL, stored, cfg.in_channels, cfg.dims, seed=5, out_channels=cfg.out_channels)
    idx = torch.tensor([1, 4, 4, 3], dtype=torch.int64, device=dev)
    return ResidentBatch(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), idx, aug, crop)


@pytest.mark.parametrize("kw", [dict(out_channels=1), dict(out_channels=3), dict(out_channels=1, dtype="fp32")],
                         ids=["bf16-K1", "bf16-K3", "fp32-K1"])
def test_executor_step_on_a_cropping_resident_batch(cuda_dev, kw):
    """fwd_bwd on a ResidentBatch carrying origins (img 32 from stored 48) == fwd_bwd on the
    tensors cropped and augmented beforehand, at the same dropout seed: the same loss-sum bits
    and gradient bits."""
    cfg, flat, be = _backend(cuda_dev, **kw)
    code = torch.tensor([5, 2, 7, 0], dtype=torch.int32, device=cuda_dev)
    org = torch.tensor([[0, 16, 3], [0, 0, 0], [0, 7, 16], [0, 9, 5]], dtype=torch.int32, device=cuda_dev)
    rb = _resident(cuda_dev, cfg, (code, None), (org, (1, 32, 32)))
    assert rb.npix == 4 * 32 * 32 * cfg.out_channels
    be.fwd_bwd(rb, None, seed=77)
    torch.cuda.synchronize()
    s1, g1 = be.sums().clone(), flat.grad.clone()
    x, y = rb.tensors()
    assert tuple(x.shape) == (4, 32, 32, 4) and torch.equal(x[3], rb.x_all[3, 9:41, 5:37])
    be.fwd_bwd(x.contiguous(), y.contiguous(), seed=77)
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all() and g1.abs().sum() > 0
    assert torch.equal(bits(s1), bits(be.sums())) and torch.equal(bits(g1), bits(flat.grad))
    # origins alone (--crop without --augment): the same launch with a null code
    rb2 = _resident(cuda_dev, cfg, None, (org, (1, 32, 32)))
    be.fwd_bwd(rb2, None, seed=78)
    torch.cuda.synchronize()
    s2, g2 = be.sums().clone(), flat.grad.clone()
    x2, y2 = rb2.tensors()
    be.fwd_bwd(x2.contiguous(), y2.contiguous(), seed=78)
    torch.cuda.synchronize()
    assert torch.equal(bits(s2), bits(be.sums())) and torch.equal(bits(g2), bits(flat.grad))


def test_gather_crop_args_refuses_wrong_tensors(cuda_dev):
    cfg, flat, be = _backend(cuda_dev, out_channels=1)
    e = be.engine
    org = torch.zeros(4, 3, dtype=torch.int32, device=cuda_dev)
    rb = _resident(cuda_dev, cfg, None, None)
    for crop in ((org.long(), (1, 32, 32)), (org[:3], (1, 32, 32)), (org.cpu(), (1, 32, 32)), (org, (1, 16, 16)),
                 (org.t().contiguous().t(), (1, 32, 32))):
        with pytest.raises(ValueError):
            e.load_indexed(rb.x_all, rb.y_all, rb.idx, crop=crop)
    with pytest.raises(ValueError):
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(torch.zeros(4, device=cuda_dev), None), crop=(org, (1, 32, 32)))


def test_resident_feeder_uploads_the_origins_with_the_indices(cuda_dev):
    """DeviceFeeder on resident data with a patch: the origins are drawn for the sorted indices
    and reach the device unchanged in the one upload; the lazy batch, its tensors and the
    non-lazy batch are the same cropped, augmented batch; an executor takes the lazy batch."""
    from unet_distributed_amd.data.datasets import foreground_table
    from unet_distributed_amd.data.loader import DeviceFeeder
    cfg, flat, be = _backend(cuda_dev, out_channels=1)
    rb0 = _resident(cuda_dev, cfg, None, None)
    xs, ys = rb0.x_all.cpu().numpy(), rb0.y_all.cpu().numpy()
    f = DeviceFeeder(xs, ys, 4, cuda_dev, mode="on", patch=(1, 32, 32))
    assert f.resident
    table = foreground_table(ys)
    idx = [3, 1, 4, 4]

    def aug(si):
        code, aff = A.draw(3, 5, si, "flip,rot90,intensity", 4, 2, 0.2)
        return code, aff, A.draw_crop(3, 5, si, (1, 48, 48), (1, 32, 32), "foreground", 1.0, table)[0]

    code, aff, org = aug(np.array(sorted(idx)))
    rb, none = f.get(idx, lazy=True, aug=aug)
    assert none is None and rb.idx.tolist() == sorted(idx) and rb.idx.dtype == torch.int64
    assert rb.aug[0].dtype == torch.int32 and rb.aug[0].cpu().tolist() == code.tolist()
    assert torch.equal(rb.aug[1].cpu(), torch.from_numpy(aff))
    assert rb.crop[0].dtype == torch.int32 and rb.crop[0].is_contiguous() and tuple(rb.crop[1]) == (1, 32, 32)
    assert torch.equal(rb.crop[0].cpu(), torch.from_numpy(org)) and rb.npix == 4 * 32 * 32
    x, y = f.get(idx, aug=aug)
    tx, ty = rb.tensors()
    wx, wy = A.apply_torch(*A.crop_torch(rb0.x_all[sorted(idx)], rb0.y_all[sorted(idx)], org, (1, 32, 32)), code, aff)
    assert torch.equal(x, wx) and torch.equal(y, wy) and torch.equal(tx, wx) and torch.equal(ty, wy)
    be.engine.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=rb.aug, crop=rb.crop)
    torch.cuda.synchronize()
    got = be.engine.bufs["x"].view(wx.shape).float()
    assert (got - wx).abs().max() <= 2.0 ** -8 * wx.abs().max()         # (bf16 of the same pixels)
    assert torch.equal(be.engine.target.view(wy.shape).float(), wy)


def test_cli_trains_on_patches_and_evaluates_through_sliding_windows(cuda_dev, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "--synthetic_size", "48", "--img_size", "32",
           "--in_channels", "4", "--batch_size", "8", "--synthetic_train", "16", "--synthetic_test", "12",
           "--crop", "foreground", "--augment", "flip,rot90", "--eval_hd95", "--steps", "3", "--no_checkpoint",
           "--notensorboard", "--noexport", "--log_jsonl", str(tmp_path / "m.jsonl")]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout
    assert "backend native" in out and "Training patches: 32 x 32 of 48 x 48, foreground 0.33" in out, out[-3000:]
    assert "Evaluation: sliding window, overlap 0.5, gaussian" in out
    assert "class 0: Dice = " in out and "class 0: HD95 = " in out and "(12 cases)" in out, out[-3000:]
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    final = [q for q in recs if q["kind"] == "test_final"]
    assert len(final) == 1 and final[0]["sliding"] == {"overlap": 0.5, "blend": "gaussian"}
    assert final[0]["cases"] == 12 and final[0]["batches"] == 1 and "hd95" in final[0]["per_class"]
    assert all(np.isfinite(final[0][k]) for k in ("loss", "dice", "sensitivity", "specificity"))

"""Multi-class Mask head (n_cl_out 2..4) on the GPU: the K-class head kernels
(csrc/kernels/head_mc.hip) and the K-channel batch gather against fp32 ATen, and the whole
step / optimiser / training / inference paths through the HIP executor against the fp32
ATen reference.

Whole-step parity measured on an MI355X (1 - cosine kernel / bias, norm-ratio deviation,
whole-gradient distance), next to the single-class step at the same shape with the three
head fusions off -- see profiles/r7_multiclass.md for the records.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PAD = 4096              # guard elements on each side of an output


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


class Guarded:
    """An output of `n` elements in the middle of a NaN-filled buffer: after the launch the
    payload is finite and the guard rows are still NaN."""

    def __init__(self, n, dtype, dev):
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=dev)
        self.out = self.buf[PAD:PAD + n]

    def check(self):
        assert torch.isfinite(self.out.float()).all()
        assert torch.isnan(self.buf[:PAD].float()).all() and torch.isnan(self.buf[PAD + self.out.numel():].float()).all()


def _head_case(dev, Cc, K, P, dt, seed):
    torch.manual_seed(seed)
    x = F.relu(torch.randn(P, Cc, device=dev)).to(dt)
    w = torch.randn(Cc, K, device=dev) * 0.3
    b = torch.randn(K, device=dev)
    t = (torch.rand(P, K, device=dev) > 0.7).to(dt)
    return x, w, b, t


def _head_run(dev, x, w, b, t, loss, gscale, dtype_id):
    """head_fwd + head_bwd of the K-class head into guarded outputs."""
    P, Cc = x.shape
    K = w.shape[1]
    nb = C().head_blocks(P)
    prob = Guarded(P * K, torch.float32, dev)
    part = torch.zeros(nb * (Cc + 1) * K + 4 * nb, device=dev)
    sums = Guarded(4, torch.float32, dev)
    C().generic("head_fwd", [ptr(x), ptr(w), ptr(b), ptr(t), ptr(prob.out), ptr(part), ptr(sums.out)], [P, Cc, K], [],
                stream(), dtype=dtype_id)
    dx = Guarded(P * Cc, x.dtype, dev)
    gw = Guarded(Cc * K, torch.float32, dev)
    gb = Guarded(K, torch.float32, dev)
    bce_w = 0.5 if loss == "dice_bce" else 0.0
    C().generic("head_bwd", [ptr(x), ptr(w), ptr(prob.out), ptr(t), ptr(sums.out), ptr(dx.out), ptr(part), ptr(gw.out),
                             ptr(gb.out)], [P, Cc, K], [1.0 / (P * K), bce_w, gscale], stream(), dtype=dtype_id)
    torch.cuda.synchronize()
    return prob, sums, dx, gw, gb


@pytest.mark.parametrize("loss", ["dice", "dice_bce"])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("Cc", [32, 64])
def test_multiclass_head_fwd_bwd(cuda_dev, Cc, K, loss):
    """P = 1001: odd, no multiple of the block or of 4 (grid-stride tail; a K = 3 row is 12 /
    6 bytes).  Bounds of the single-class head test; reference: autograd through
    ops.losses.total_loss on [P, K] logits."""
    from unet_distributed_amd.ops.losses import total_loss
    P, gscale = 1001, 8.0
    x, w, b, t = _head_case(cuda_dev, Cc, K, P, torch.bfloat16, 10 + Cc + K)
    prob, sums, dx, gw, gb = _head_run(cuda_dev, x, w, b, t, loss, gscale, 0)
    xr = x.float().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    z = xr @ wr + br
    tf = t.float()
    lossv, p = total_loss(tf, z, loss, 0.5)
    I, St, Sp = (tf * p).sum(), tf.sum(), p.sum()
    bce = F.binary_cross_entropy_with_logits(z, tf, reduction="sum")
    gx, gwr, gbr = torch.autograd.grad(lossv * gscale, [xr, wr, br])
    errs = dict(prob=rel_err(prob.out.view(P, K), p), sums=rel_err(sums.out, torch.stack([I, St, Sp, bce])),
                dx=rel_err(dx.out.view(P, Cc), gx * (x.float() > 0)), gw=rel_err(gw.out.view(Cc, K), gwr),
                gb=rel_err(gb.out, gbr))
    print("head_mc", Cc, K, loss, json.dumps(errs))
    for g in (prob, sums, dx, gw, gb):
        g.check()
    assert errs["prob"] < 1e-4 and errs["sums"] < 1e-4
    assert errs["dx"] < 1e-2
    assert errs["gw"] < 1e-3 and errs["gb"] < 1e-3


def test_multiclass_head_fp16_device_loss_scale(cuda_dev):
    """The fp16 build, the loss scale read from device memory (the trainer's path), more than
    one grid-stride round (P > 1024 blocks x 256)."""
    from unet_distributed_amd.ops.losses import total_loss
    dev, P, Cc, K = cuda_dev, 1024 * 256 + 77, 32, 3
    x, w, b, t = _head_case(dev, Cc, K, P, torch.float16, 5)
    nb = C().head_blocks(P)
    prob = torch.empty(P * K, device=dev)
    part = torch.zeros(nb * (Cc + 1) * K + 4 * nb, device=dev)
    sums = torch.empty(4, device=dev)
    C().generic("head_fwd", [ptr(x), ptr(w), ptr(b), ptr(t), ptr(prob), ptr(part), ptr(sums)], [P, Cc, K], [],
                stream(), dtype=1)
    dx = torch.empty_like(x)
    gw, gb = torch.empty(Cc * K, device=dev), torch.empty(K, device=dev)
    scale = torch.full((1,), 4096.0, device=dev)
    C().generic("head_bwd", [ptr(x), ptr(w), ptr(prob), ptr(t), ptr(sums), ptr(dx), ptr(part), ptr(gw), ptr(gb),
                             ptr(scale)], [P, Cc, K], [1.0 / (P * K), 0.0, 1.0], stream(), dtype=1)
    xr = x.float().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    lossv, p = total_loss(t.float(), xr @ wr + b, "dice", 1.0)
    gx, gwr = torch.autograd.grad(lossv, [xr, wr])
    assert rel_err(prob.view(P, K), p) < 1e-4
    assert rel_err(dx.float() / 4096.0, gx * (x.float() > 0)) < 2e-3
    assert rel_err(gw.view(Cc, K) / 4096.0, gwr) < 1e-3


def test_multiclass_head_predict_path_without_target(cuda_dev):
    """t == nullptr: probabilities and Sp only."""
    dev, P, Cc, K = cuda_dev, 1001, 32, 3
    x, w, b, t = _head_case(dev, Cc, K, P, torch.bfloat16, 6)
    prob = Guarded(P * K, torch.float32, dev)
    part = torch.zeros(C().head_blocks(P) * ((Cc + 1) * K + 4), device=dev)
    sums = torch.empty(4, device=dev)
    C().generic("head_fwd", [ptr(x), ptr(w), ptr(b), 0, ptr(prob.out), ptr(part), ptr(sums)], [P, Cc, K], [], stream())
    torch.cuda.synchronize()
    p = torch.sigmoid(x.float() @ w + b)
    prob.check()
    assert rel_err(prob.out.view(P, K), p) < 1e-4
    s = sums.cpu()
    assert s[0] == 0 and s[1] == 0 and s[3] == 0 and abs(s[2].item() - p.sum().item()) < 1e-4 * p.sum().item()


def test_multiclass_head_bwd_is_deterministic(cuda_dev):
    x, w, b, t = _head_case(cuda_dev, 64, 3, 20011, torch.bfloat16, 7)
    a = _head_run(cuda_dev, x, w, b, t, "dice_bce", 3.0, 0)
    c = _head_run(cuda_dev, x, w, b, t, "dice_bce", 3.0, 0)
    for u, v in zip(a[2:], c[2:]):
        assert torch.equal(u.out, v.out)


def test_gather_batch_three_target_channels(cuda_dev):
    dev, N, B, P, cin, cpad, K = cuda_dev, 8, 5, 37 * 3, 4, 4, 3
    torch.manual_seed(8)
    x_all = torch.randn(N, P, cin, device=dev)
    y_all = (torch.rand(N, P, K, device=dev) > 0.5).float()
    idx = torch.tensor([6, 0, 3, 7, 2], device=dev, dtype=torch.int64)
    xb = Guarded(B * P * cpad, torch.bfloat16, dev)
    tb = Guarded(B * P * K, torch.bfloat16, dev)
    C().generic("gather_batch", [ptr(x_all), ptr(y_all), ptr(idx), ptr(xb.out), ptr(tb.out)], [B, P, cin, cpad, K], [],
                stream())
    torch.cuda.synchronize()
    xb.check()
    tb.check()
    assert torch.equal(xb.out.view(B, P, cpad), x_all.index_select(0, idx).bfloat16())
    assert torch.equal(tb.out.view(B, P, K), y_all.index_select(0, idx).bfloat16())
    # a padded input (cin 3 -> cpad 4: pad channel zero)
    x3 = x_all[..., :3].contiguous()
    xb = Guarded(B * P * cpad, torch.bfloat16, dev)
    C().generic("gather_batch", [ptr(x3), ptr(y_all), ptr(idx), ptr(xb.out), ptr(tb.out)], [B, P, 3, cpad, K], [],
                stream())
    torch.cuda.synchronize()
    want = torch.zeros(B, P, cpad, device=dev, dtype=torch.bfloat16)
    want[..., :3] = x3.index_select(0, idx).bfloat16()
    assert torch.equal(xb.out.view(B, P, cpad), want)


# ------------------------------------------------------------------ whole step
def _setup(cuda_dev, opts=None, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend, TorchBackend
    from unet_distributed_amd.runtime.native_engine import NativeUNet
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(**kw)
    spec = spec_from_config(cfg)
    B = cfg.batch_size
    x, y = synthetic_brats(B, cfg.img_size, cfg.in_channels, cfg.dims, seed=5, out_channels=cfg.out_channels)
    x, y = torch.from_numpy(x).to(cuda_dev), torch.from_numpy(y).to(cuda_dev)
    init = reference.init_params(spec, seed=3)
    fn = FlatParams(spec, device=cuda_dev)
    fn.load_dict(init)
    nb = NativeBackend(spec, fn, cfg, cuda_dev, B)
    if opts:
        # engine options are not a trainer flag: rebuild the backend's executor with them
        nb.engine = NativeUNet(spec, fn, B, cfg.img_size, cuda_dev, loss=cfg.loss, bce_weight=cfg.bce_weight,
                               eval_dropout=cfg.eval_dropout, dtype=cfg.dtype, opts=opts)
    cfg32 = Config(**dict(kw, dtype="fp32"))
    ft = FlatParams(spec, device=cuda_dev)
    ft.load_dict(init)
    tb = TorchBackend(spec, ft, cfg32, cuda_dev, B)
    return spec, cfg, x, y, fn, nb, ft, tb


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _grad_parity(fn, ft, tag, scale=1.0):
    rows = {}
    for name, shape, off, n in fn.entries:
        gn, gt = fn.grad[off:off + n] / scale, ft.grad[off:off + n]
        rows[name] = (1.0 - _cos(gn, gt), abs((gn.norm() / (gt.norm() + 1e-30)).item() - 1.0))
    worst_k = max((v[0], k) for k, v in rows.items() if not k.endswith("/bias"))
    worst_b = max((v[0], k) for k, v in rows.items() if k.endswith("/bias"))
    worst_r = max((v[1], k) for k, v in rows.items())
    rec = dict(tag=tag, worst_cos_dist_kernel=worst_k, worst_cos_dist_bias=worst_b, worst_ratio_dev=worst_r,
               total_cos_dist=1.0 - _cos(fn.grad / scale, ft.grad))
    print("parity", json.dumps(rec))
    log = os.environ.get("UNET_PARITY_JSONL")      # optional: a file the records are appended to
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(rec) + "\n")
    return rows, rec


def _check_parity(rows, rec):
    """The project's caps (tests/test_gpu_model.py _check_parity defaults)."""
    for name, (dc, dr) in rows.items():
        assert dc < (0.05 if name.endswith("/bias") else 0.02), (rec["tag"], name, dc)
        assert dr < 0.1, (rec["tag"], name, dr)
    assert rec["total_cos_dist"] < 0.01, rec


def _step(cuda_dev, tag, scale, opts=None, **kw):
    spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, opts=opts, **kw)
    nb.fwd_bwd(x, y, seed=77, grad_scale=scale)
    tb.fwd_bwd(x, y, seed=77)
    torch.cuda.synchronize()
    assert torch.isfinite(fn.grad).all()
    sn, st = nb.sums().cpu(), tb.sums().cpu()
    rows, rec = _grad_parity(fn, ft, tag, scale)
    return nb, sn, st, rows, rec


STEP_CASES = [
    dict(out_channels=3, batch_size=4, img_size=64, in_channels=4),
    dict(out_channels=2, batch_size=2, img_size=32, in_channels=4, dims=3),
    dict(out_channels=4, batch_size=2, img_size=64, in_channels=4, use_upsampling=True, loss="dice_bce"),
    dict(out_channels=3, batch_size=4, img_size=64, in_channels=4, dtype="fp16"),
]


@pytest.mark.parametrize("kw", STEP_CASES, ids=lambda kw: "K%d-%s" % (kw["out_channels"], kw.get("dtype", "bf16")))
def test_multiclass_step_matches_reference(cuda_dev, kw):
    """The K-class step against the fp32 ATen step, and beside it the single-class step at the
    same shape on the same (unfused) head path: its record is the like-for-like baseline."""
    scale = 4096.0 if kw.get("dtype") == "fp16" else 1.0     # the static scale of the fp16 tests
    tag = ",".join("%s=%s" % kv for kv in sorted(kw.items()))
    nb, sn, st, rows, rec = _step(cuda_dev, "mc:" + tag, scale, **kw)
    e = nb.engine
    assert e.K == kw["out_channels"] and not any(e.fusions.get(n) for n in ("head_fuse", "head_onload", "head_wsum"))
    kw1 = dict(kw, out_channels=1)
    nb1, sn1, st1, rows1, rec1 = _step(cuda_dev, "mc-k1-unfused:" + ",".join("%s=%s" % kv for kv in sorted(kw1.items())),
                                       scale, opts=dict(head_fuse=0, head_onload=0, head_wsum=0), **kw1)
    assert not any(nb1.engine.fusions.get(n) for n in ("head_fuse", "head_onload", "head_wsum"))
    assert torch.allclose(sn[:3], st[:3], rtol=3e-2, atol=1.0), (sn, st)
    _check_parity(rows, rec)


def test_multiclass_adam_updates_the_mask_parameters(cuda_dev):
    from unet_distributed_amd.runtime.optim import adam_reference_
    spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, out_channels=3, batch_size=2, img_size=32, in_channels=4)
    assert fn.view(fn.master, "Mask/kernel").numel() == 32 * 3 and fn.view(fn.master, "Mask/bias").numel() == 3
    g = torch.randn(fn.numel, device=cuda_dev) * 1e-2
    fn.grad.copy_(g)
    w0 = fn.master.clone()
    nb.adam_step(5e-4, 0.9, 0.999)
    w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    adam_reference_(w, g, m, v, 5e-4, 0.9, 0.999)
    torch.cuda.synchronize()
    for name in ("Mask/kernel", "Mask/bias"):
        got, want = fn.view(fn.master, name), fn.view(w, name)
        assert not torch.equal(got, fn.view(w0, name))
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-7), name
    assert torch.allclose(fn.master, w, rtol=1e-5, atol=1e-7)


def test_multiclass_training_reduces_loss(cuda_dev):
    """30 steps on one synthetic batch with three nested output regions, HIP graphs on."""
    from unet_distributed_amd.runtime.optim import TFAdam
    from unet_distributed_amd.runtime.trainer import _NativeOpt
    spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, out_channels=3, batch_size=8, img_size=32, in_channels=4,
                                              synthetic=True, learning_rate=1e-3, hip_graph=True)
    assert nb.engine.graphs is not None
    opt = TFAdam(fn, cfg, native=_NativeOpt(nb))
    losses = []
    for i in range(30):
        nb.fwd_bwd(x, y, seed=i)
        opt.step()
        s = nb.sums().cpu()
        losses.append((-torch.log(2 * s[0] + 1) + torch.log(s[1] + s[2] + 1)).item())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    imgs = nb.summary_images(3)
    assert imgs["predictions"].shape == (3, 32, 32) and imgs["ground_truth"].shape == (3, 32, 32)


def test_multiclass_resident_batches_and_eval(cuda_dev):
    """load_indexed (the trainer's HBM-resident path) gives the step load_batch gives, and
    eval_sums runs the K-class inference plan."""
    from unet_distributed_amd.data.loader import ResidentBatch
    spec, cfg, x, y, fn, nb, ft, tb = _setup(cuda_dev, out_channels=3, batch_size=4, img_size=32, in_channels=4)
    nb.fwd_bwd(x, y, seed=5)
    g0, s0 = fn.grad.clone(), nb.sums().clone()
    perm = torch.tensor([2, 0, 3, 1], device=cuda_dev)
    inv = torch.argsort(perm)
    nb.fwd_bwd(ResidentBatch(x[perm].contiguous(), y[perm].contiguous(), inv), None, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(fn.grad, g0) and torch.equal(nb.sums(), s0)
    se, st = nb.eval_sums(x, y).cpu(), tb.eval_sums(x, y).cpu()
    assert torch.allclose(se[:3], st[:3], rtol=3e-2, atol=1.0), (se, st)


def test_multiclass_inference_export_roundtrip(cuda_dev, tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=64, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    d = export_model(cfg, spec, flat)
    model = load_saved_model(d, device=cuda_dev, batch=4)
    assert model.name == "native" and model.spec.n_cl_out == 3
    x, _ = synthetic_brats(6, 64, 4, seed=2)
    p = model.predict(x)
    assert p.shape == (6, 64, 64, 3)
    with torch.no_grad():
        ref = reference.forward(spec, {k: v.to(cuda_dev) for k, v in flat.params().items()},
                                torch.from_numpy(x).to(cuda_dev), train=False, dropout=False).cpu().numpy()
    assert np.abs(p - ref).max() < 0.05, np.abs(p - ref).max()

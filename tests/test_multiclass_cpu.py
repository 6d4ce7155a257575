"""Multi-class Mask head (--out_channels 2..4), the parts that need no GPU: backend
resolution, the dry-run plans of the HIP executor (runtime/plan_check.py), the nested
synthetic masks, update_channels mode 5 and the export / load round trip."""
import itertools
import os

import numpy as np
import pytest
import torch

from unet_distributed_amd.config import Config, validate
from unet_distributed_amd.data.datasets import synthetic_brats, update_channels
from unet_distributed_amd.models import reference
from unet_distributed_amd.models.spec import UNetSpec, spec_from_config
from unet_distributed_amd.parallel.grad_sync import plan_buckets
from unet_distributed_amd.runtime import native_engine as ne
from unet_distributed_amd.runtime.backends import resolve_backend
from unet_distributed_amd.runtime.params import FlatParams
from unet_distributed_amd.runtime.plan_check import check_engine

HEAD_FUSIONS = ("head_fuse", "head_onload", "head_wsum")


@pytest.mark.parametrize("K", [2, 3, 4])
def test_multiclass_resolves_to_native(K):
    """device 'cuda' is only a device type here: nothing touches a GPU."""
    for kw in (dict(), dict(dtype="fp16"), dict(dims=3, img_size=32), dict(use_upsampling=True)):
        cfg = Config(dtype=kw.pop("dtype", "bf16"), in_channels=4, out_channels=K, **kw)
        assert resolve_backend("auto", spec_from_config(cfg), cfg, "cuda") == "native"


@pytest.mark.parametrize("kw,why", [(dict(out_channels=3, norm="batch"), "norm=batch"),
                                    (dict(out_channels=2, norm="group"), "norm=group"),
                                    (dict(out_channels=3, dtype="fp32"), "fp32"),
                                    (dict(out_channels=5), "n_cl_out=5")])
def test_unsupported_multiclass_configs_name_their_reason(kw, why):
    cfg = Config(in_channels=4, **kw)
    spec = spec_from_config(cfg)
    for want in ("auto", "native"):
        with pytest.raises(RuntimeError, match=why):
            resolve_backend(want, spec, cfg, "cuda")
    assert resolve_backend("torch", spec, cfg, "cuda") == "torch"


def test_config_validate_bounds_out_channels():
    validate(Config(out_channels=4))
    validate(Config(out_channels=3, mode=5))
    for bad in (Config(out_channels=0), Config(out_channels=5), Config(out_channels=4, mode=5)):
        with pytest.raises(SystemExit):
            validate(bad)


def _engine(K, ups, dims, img=32, batch=2, dtype="bf16"):
    spec = UNetSpec(in_channels=1 if ups else 4, n_cl_out=K, use_upsampling=ups, dims=dims)
    flat = FlatParams(spec)
    return ne.NativeUNet(spec, flat, batch, img, "cpu", bucket_bounds=plan_buckets(flat, 4.0), dry_run=True,
                         dtype=dtype)


@pytest.mark.parametrize("K,dims,ups", list(itertools.product((2, 3, 4), (2, 3), (False, True))))
def test_multiclass_plans_validate(K, dims, ups):
    """Def-use, write extents, every launch resolves, every parameter gradient written; the
    single-class head fusions are not applied, and plan validation names why."""
    e = _engine(K, ups, dims)
    assert check_engine(e) == {"train": [], "eval": []}
    for name in HEAD_FUSIONS:
        assert name not in e.fusions
        assert ne.FUSIONS[name].unmet(e) and not e._fusion_ok(name)
    names = e.plan.names()
    assert names.count("fwd:Mask") == 1 and names.count("bwd:Mask") == 1 and "wgrad:Mask" not in names
    assert "fwd:Mask" in e.eval_plan.names()
    P = e.npix(1)
    assert e.prob.numel() == P * K and e.target.numel() == P * K
    assert tuple(e.probs().shape[-1:]) == (K,)
    ops = {op["name"]: op for op in e.plan.ops}
    assert (int(e.prob.data_ptr()), P * K * 4) in ops["fwd:Mask"]["spans"]
    hc = e.tinfo[e.head_in][1]
    assert (e.grad_ptr("Mask/kernel"), hc * K * 4) in ops["bwd:Mask"]["spans"]
    assert (e.grad_ptr("Mask/bias"), K * 4) in ops["bwd:Mask"]["spans"]
    # the other fusions of the shape are those of the single-class plan
    e1 = _engine(1, ups, dims)
    assert sorted(set(e1.fusions) - set(HEAD_FUSIONS)) == sorted(e.fusions)


def test_multiclass_fp16_plan_validates():
    e = _engine(3, False, 2, dtype="fp16")
    assert check_engine(e) == {"train": [], "eval": []} and e.dt_id == 1


@pytest.mark.parametrize("dims,ups", list(itertools.product((2, 3), (False, True))))
def test_single_class_plans_keep_their_head_fusions(dims, ups):
    e = _engine(1, ups, dims)
    assert check_engine(e) == {"train": [], "eval": []}
    assert e.fusions.get("head_fuse") == ["conv9b"]
    if dims == 2:
        assert e.fusions.get("head_onload") == ["conv9b"]
        assert "wgrad:Mask" in e.plan.names()
    # the single-class head ops carry no class count: the recorded plan is what it was
    assert e._head_k() == []


def test_single_class_128_plan_keeps_head_wsum():
    e = _engine(1, False, 2, img=128)
    assert all(e.fusions.get(n) == ["conv9b"] for n in HEAD_FUSIONS)


def test_executor_refuses_what_the_head_kernels_do_not_cover():
    for kw in (dict(n_cl_out=5), dict(n_cl_out=3, norm="batch")):
        spec = UNetSpec(in_channels=4, **kw)
        with pytest.raises(NotImplementedError):
            ne.NativeUNet(spec, FlatParams(spec), 2, 32, "cpu", dry_run=True)


def test_multiclass_head_ops_are_checked_at_plan_time():
    """The generic head ops reject class counts / channels no kernel takes and launches whose
    flat indices leave 32 bits (ValueError, nothing is launched)."""
    from unet_distributed_amd import native
    C = native.require()
    p = C.Plan(0)
    p.add_generic("head_fwd", [1] * 7, [1001, 32, 3], [], "ok")
    p.add_generic("head_bwd", [1] * 9, [1001, 64, 4], [1.0, 0.0, 1.0], "ok")
    p.add_generic("gather_batch", [1] * 5, [2, 64, 4, 4, 3], [], "ok")
    assert p.check_dispatch(0, p.size()) == []
    for ints in ([1001, 32, 5], [1001, 16, 2], [1 << 30, 32, 2], [1 << 29, 64, 3]):
        with pytest.raises(ValueError):
            p.add_generic("head_fwd", [1] * 7, ints, [], "bad")
        with pytest.raises(ValueError):
            p.add_generic("head_bwd", [1] * 9, ints, [1.0, 0.0, 1.0], "bad")
    with pytest.raises(ValueError):          # the multi-class backward always writes dx
        p.add_generic("head_bwd", [1] * 5 + [0] + [1] * 3, [1001, 32, 3], [1.0, 0.0, 1.0], "bad")
    with pytest.raises(ValueError):
        p.add_generic("gather_batch", [1] * 5, [1 << 15, 1 << 14, 4, 4, 4], [], "bad")
    with pytest.raises(ValueError):
        p.add_generic("gather_batch", [1] * 5, [2, 64, 4, 4, 5], [], "bad")


@pytest.mark.parametrize("difficulty", ["easy", "hard"])
def test_synthetic_nested_masks(difficulty):
    """Images and channel 0 do not depend on out_channels; the channels are nested; the
    innermost region is not empty everywhere."""
    inner = 0
    for seed in range(3):
        x1, y1 = synthetic_brats(8, 32, 4, seed=seed, difficulty=difficulty)
        x3, y3 = synthetic_brats(8, 32, 4, seed=seed, difficulty=difficulty, out_channels=3)
        assert y1.shape == (8, 32, 32, 1) and y3.shape == (8, 32, 32, 3)
        assert np.array_equal(x1, x3) and np.array_equal(y1[..., 0], y3[..., 0])
        assert set(np.unique(y3)) <= {0.0, 1.0}
        for k in range(2):
            assert (y3[..., k + 1] <= y3[..., k]).all()
        assert y3[..., 1].sum() < y3[..., 0].sum()
        inner += int((y3[..., 2].reshape(8, -1).sum(1) > 0).sum())
    assert inner >= 1
    x4, y4 = synthetic_brats(4, 32, 4, seed=0, difficulty=difficulty, out_channels=4)
    assert y4.shape[-1] == 4 and (y4[..., 3] <= y4[..., 2]).all()
    with pytest.raises(ValueError):
        synthetic_brats(2, 32, 4, out_channels=5)


def test_synthetic_nested_masks_3d():
    x1, y1 = synthetic_brats(2, 16, 4, dims=3, seed=1)
    x2, y2 = synthetic_brats(2, 16, 4, dims=3, seed=1, out_channels=2)
    assert y2.shape == (2, 16, 16, 16, 2)
    assert np.array_equal(x1, x2) and np.array_equal(y1[..., 0], y2[..., 0])
    assert (y2[..., 1] <= y2[..., 0]).all()


def test_update_channels_mode5_and_the_reference_modes():
    rng = np.random.default_rng(0)
    imgs = rng.standard_normal((3, 8, 8, 4)).astype(np.float32)
    msks = (rng.random((3, 8, 8, 4)) > 0.7).astype(np.float32)
    whole = msks.sum(-1)
    core = msks[..., 0] + msks[..., 2] + msks[..., 3]
    enh = msks[..., 3]
    for K in (1, 2, 3):
        x, y = update_channels(imgs, msks, 4, K, 5)
        assert x.dtype == np.float32 and y.shape == (3, 8, 8, K)
        assert np.array_equal(x, imgs)
        for k, want in enumerate((whole, core, enh)[:K]):
            assert np.array_equal(y[..., k], want)
    with pytest.raises(ValueError):
        update_channels(imgs, msks, 4, 4, 5)
    # modes 1-4: what they were (the reference fills channel 0 only)
    want = {1: (imgs[..., 2], whole), 2: (imgs[..., 0], enh), 3: (imgs[..., 1], core)}
    for mode, (xi, yi) in want.items():
        x, y = update_channels(imgs, msks, 1, 1, mode)
        assert np.array_equal(x[..., 0], xi) and np.array_equal(y[..., 0], yi)
    x, y = update_channels(imgs, msks, 4, 1, 4)
    assert np.array_equal(x, imgs) and np.array_equal(y[..., 0], whole)
    x, y = update_channels(imgs, msks, 1, 3, 1)
    assert np.array_equal(y[..., 0], whole) and not y[..., 1:].any()


def test_multiclass_export_roundtrip_cpu(tmp_path):
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    d = export_model(cfg, spec, flat)
    os.remove(os.path.join(d, "saved_model.json"))          # the GraphDef alone describes the model
    model = load_saved_model(d, device="cpu")
    assert model.spec.n_cl_out == 3 and model.name == "torch"
    x, _ = synthetic_brats(3, 32, 4, seed=2, out_channels=3)
    p = model.predict(x)
    assert p.shape == (3, 32, 32, 3)
    with torch.no_grad():
        ref = reference.forward(spec, flat.params(), torch.from_numpy(x), train=False, dropout=False).numpy()
    assert np.allclose(p, ref, atol=1e-5)

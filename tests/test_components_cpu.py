"""Connected-component post-processing off the GPU: the torch definition (ops/components.py)
on hand-written answers and against scipy, the --eval_components flag, plan-time validation of
the components op and dry-run executors, and the ATen backend, trainer report, Predictor and
sanity_check with the option on."""
import contextlib
import io
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from unet_distributed_amd.ops import seg_metrics
from unet_distributed_amd.ops.components import components_torch, describe, labels_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(mask_or_prob, thr=0.5, largest=False, min_size=0):
    """(out [grid], info list of 4, labels [grid]) of one K = 1 sample on its own grid."""
    p = torch.as_tensor(np.asarray(mask_or_prob, dtype=np.float32))[None, ..., None]
    out, info = components_torch(p, thr, largest, min_size)
    assert out.dtype == torch.float32 and info.dtype == torch.int32 and info.shape == (1, 1, 4)
    return out[0, ..., 0], info[0, 0].tolist(), labels_torch(p, thr)[0, 0]


# ------------------------------------------------------------------ hand cases
@pytest.mark.parametrize("grid", [(4, 6), (3, 4, 5)])
def test_empty_full_and_single_voxel(grid):
    S = int(np.prod(grid))
    z = np.zeros(grid)
    out, info, lab = _run(z, largest=True, min_size=3)
    assert info == [0, 0, 0, 0] and (lab == -1).all() and torch.equal(out, torch.zeros(grid))
    out, info, lab = _run(np.ones(grid), largest=True, min_size=S)
    assert info == [1, 1, S, S] and (lab == 0).all() and torch.equal(out, torch.ones(grid))
    one = z.copy()
    at = tuple(v - 1 for v in grid)
    one[at] = 0.75
    out, info, lab = _run(one, largest=True)
    assert info == [1, 1, 1, 1] and lab[at] == S - 1 and (lab == -1).sum() == S - 1
    assert out[at] == 0.75 and out.sum() == 0.75
    out, info, _ = _run(one, min_size=2)
    assert info == [1, 0, 1, 0] and out.sum() == 0.0


def test_diagonal_contact_does_not_connect_and_the_border_does_not_wrap():
    m = np.zeros((4, 5))
    m[0, 0] = m[1, 1] = 1                    # diagonal neighbours
    m[2, 4] = m[3, 0] = 1                    # adjacent in memory (end of a row, start of the next)
    m[0, 4] = 1                              # the other end of row 0
    _, info, lab = _run(m)
    assert info == [5, 5, 1, 5]
    assert [lab[0, 0].item(), lab[1, 1].item(), lab[2, 4].item(), lab[3, 0].item(), lab[0, 4].item()] == [0, 6, 14, 15, 4]


def test_equal_sizes_the_smaller_label_wins():
    m = np.zeros((6, 8))
    m[4:6, 5:7] = 1                          # label 37
    m[1:3, 1:3] = 1                          # label 9, the same size
    m[0, 7] = 1                              # a smaller component with the smallest label
    out, info, lab = _run(m, largest=True)
    assert info == [3, 1, 4, 4]
    assert lab[1, 1] == 9 and lab[5, 6] == 37 and lab[0, 7] == 7
    want = np.zeros((6, 8), dtype=np.float32)
    want[1:3, 1:3] = 1
    assert torch.equal(out, torch.from_numpy(want))


def test_min_size_boundaries():
    m = np.zeros((5, 9))
    m[0, 0:3] = 1                            # 3 voxels
    m[2, 0:5] = 1                            # 5 voxels
    m[4, 0:2] = 1                            # 2 voxels
    assert _run(m, min_size=6)[1] == [3, 0, 5, 0]                      # larger than the largest: nothing
    assert _run(m, min_size=6)[0].sum() == 0
    assert _run(m, largest=True, min_size=6)[1] == [3, 0, 5, 0]
    assert _run(m, min_size=5)[1] == [3, 1, 5, 5]                      # equal to a size: kept
    assert _run(m, min_size=3)[1] == [3, 2, 5, 8]
    assert _run(m, largest=True, min_size=3)[1] == [3, 1, 5, 5]
    out = _run(m, min_size=3)[0]
    assert out[0, :3].sum() == 3 and out[2, :5].sum() == 5 and out[4].sum() == 0
    assert _run(m, min_size=0)[1] == [3, 3, 5, 10] == _run(m, min_size=1)[1]
    with pytest.raises(ValueError):
        _run(m, min_size=-1)
    for thr in (0.0, 1.0):
        with pytest.raises(ValueError):
            _run(m, thr=thr)


def test_threshold_is_inclusive_and_what_lies_below_passes_through():
    t = np.float32(0.3)
    below = np.nextafter(t, np.float32(0))
    p = np.full((3, 7), 0.123, dtype=np.float32)
    p[1, 1] = t                              # exactly at the threshold: inside
    p[1, 2] = below                          # the next float below: outside, so (1, 3) is on its own
    p[1, 3] = 0.9
    p[1, 4] = 0.9
    p[0, 6] = 0.29
    out, info, lab = _run(p, thr=0.3, largest=True)
    assert info == [2, 1, 2, 2]
    assert lab[1, 1] == 8 and lab[1, 2] == -1 and lab[1, 3] == 10
    want = p.copy()
    want[1, 1] = 0                           # removed: exactly 0.0
    assert np.array_equal(out.numpy().view(np.int32), want.view(np.int32))     # sub-threshold values bit for bit
    assert set(np.flatnonzero(out.numpy() >= t)) == {10, 11}                   # {out >= thr}: the kept component


def test_a_pair_connected_only_along_d():
    m = np.zeros((3, 4, 4))
    m[0, 1, 1] = m[1, 1, 1] = 1              # face neighbours along D
    m[2, 2, 2] = 1                           # diagonal to (1, 1, 1) in its plane and along D
    _, info, lab = _run(m)
    assert info == [2, 2, 2, 3] and lab[1, 1, 1] == 5 == lab[0, 1, 1] and lab[2, 2, 2] == 42
    assert _run(m[:, :, :, None][..., 0], largest=True)[1] == [2, 1, 2, 2]
    # the same voxels as a 2D image of one plane each never connect
    assert _run(m[0])[1] == [1, 1, 1, 1]


def test_classes_and_samples_are_separate():
    p = torch.zeros(2, 4, 5, 3)
    p[0, 0, :, 0] = 0.9                      # class 0: the first row ...
    p[0, 1, :, 1] = 0.9                      # ... class 1: the row below it: not one component
    p[0, 3, 4, 0] = 0.9                      # the last voxel of sample 0, class 0
    p[1, 0, 0, 0] = 0.9                      # the first voxel of sample 1, class 0
    p[1, 2, 1:3, 2] = 0.8
    p[1, 0, 4, 2] = 0.7
    out, info = components_torch(p, 0.5, True, 2)
    assert info.tolist() == [[[2, 1, 5, 5], [1, 1, 5, 5], [0, 0, 0, 0]], [[1, 0, 1, 0], [0, 0, 0, 0], [2, 1, 2, 2]]]
    lab = labels_torch(p, 0.5)
    assert lab.shape == (2, 3, 4, 5) and lab.dtype == torch.int64
    assert lab[0, 0, 3, 4] == 19 and lab[1, 0, 0, 0] == 0 and lab[0, 1, 1, 2] == 5 and lab[1, 2, 2, 2] == 11
    want = p.clone()
    want[0, 3, 4, 0] = 0
    want[1, 0, 0, 0] = 0
    want[1, 0, 4, 2] = 0
    assert torch.equal(out, want)
    # idempotent: the filtered map filters to itself
    again, info2 = components_torch(out, 0.5, True, 2)
    assert torch.equal(again, out) and torch.equal(info2[..., 0], info[..., 1])
    assert torch.equal(info2[..., 1], info[..., 1]) and torch.equal(info2[..., 3], info[..., 3])


def _serpentine(n):
    m = np.zeros((n, n))
    m[0::2] = 1
    for i, r in enumerate(range(1, n - 1, 2)):
        m[r, -1 if i % 2 == 0 else 0] = 1
    return m


def test_a_serpentine_is_one_component():
    m = _serpentine(33)
    _, info, lab = _run(m, largest=True)
    assert info == [1, 1, int(m.sum()), int(m.sum())] and (lab[m > 0] == 0).all()


@pytest.mark.parametrize("grid", [(8, 8), (64, 48), (16, 16, 16), (24, 6, 5)])
def test_scipy_cross_check(grid):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(sum(grid))
    for density in (0.3, 0.55, 0.8):
        p = rng.rand(*grid).astype(np.float32)
        thr = 1.0 - density
        m = p >= np.float32(thr)
        l, n = ndimage.label(m)
        idx = np.arange(m.size).reshape(grid)
        mins = np.atleast_1d(ndimage.minimum(idx, l, np.arange(1, n + 1))) if n else np.zeros(0)
        sizes = np.bincount(l.ravel(), minlength=n + 1)[1:]
        want = np.where(m, np.concatenate([[0], mins])[l], -1)
        out, info, lab = _run(p, thr=thr, largest=False, min_size=3)
        assert np.array_equal(lab.numpy(), want)
        assert info == [n, int((sizes >= 3).sum()), int(sizes.max()) if n else 0, int(sizes[sizes >= 3].sum())]
        keep = np.concatenate([[False], sizes >= 3])[l]
        assert np.array_equal(out.numpy(), np.where(m & ~keep, np.float32(0), p))


# ------------------------------------------------------------------ flag
def test_eval_components_flag_parses():
    from unet_distributed_amd.config import Config, parse_args, parse_components
    assert Config().eval_components == ""
    assert parse_components("") == (False, 0) == parse_components("  ")
    assert parse_components("largest") == (True, 0)
    assert parse_components("min:20") == (False, 20)
    assert parse_components("largest,min:20") == (True, 20) == parse_components(" min:20 , largest ")
    assert describe("largest,min:20") == "largest, min 20 voxels" and describe("min:1") == "min 1 voxels"
    assert describe("largest") == "largest"
    for bad, word in (("biggest", "unknown item 'biggest'"), ("min", "unknown item 'min'"), ("min:", "V >= 1"),
                      ("min:0", "V >= 1"), ("min:-3", "V >= 1"), ("min:2.5", "V >= 1"), ("largest,largest", "twice"),
                      ("min:2,min:3", "twice"), ("largest,", "unknown item ''"), ("min:%d" % (1 << 31), "2^31")):
        with pytest.raises(SystemExit) as err:
            parse_components(bad)
        assert "--eval_components" in str(err.value) and word in str(err.value), (bad, str(err.value))
    cfg = parse_args(["--synthetic", "--eval_components", "largest,min:20"])
    assert cfg.eval_components == "largest,min:20"
    with pytest.raises(SystemExit):
        parse_args(["--synthetic", "--eval_components", "smallest"])


# ------------------------------------------------------------------ plan-time validation (no GPU)
def _C():
    from unet_distributed_amd import native
    return native.require()


GOOD = [(3, 1, 8, 8, 1), (2, 1, 16, 24, 3), (1024, 1, 128, 128, 4), (8, 128, 128, 128, 1), (1, 1, 8, 512, 2),
        (1, 155, 240, 240, 3), (1, 1, 3, 3, 1)]


def test_components_plan_time_validation():
    from unet_distributed_amd.runtime.plan_check import components_scratch
    C = _C()
    plan = C.Plan(0)
    ptrs = [4096, 8192, 12288, 16384]
    for shape in GOOD:
        i = plan.add_generic("components", ptrs, list(shape) + [1, 20], [0.5], "components")
        assert plan.check_dispatch(i, i + 1) == []
        S = int(np.prod(shape[1:4]))
        want = -(-(shape[0] * shape[4] * (2 * S + 1 + 5 * -(-S // 16384)) * 4) // 16) * 16
        assert components_scratch(*shape) == C.components_scratch(*shape) == want
        assert C.components_check(*shape, 20) is None
    n0 = plan.size()
    bad = [((2, 1, 8, 8, 0, 1, 0), "classes"), ((2, 1, 8, 8, 5, 1, 0), "classes"),
           ((2, 1, 8, 8, 1, 1, -1), "min_size"),
           ((1, 2048, 1024, 1024, 1, 1, 0), "S = D H W"),                  # S = 2^31
           ((1 << 12, 512, 1024, 1024, 4, 0, 1), "N S K"),            # past the grid of a launch
           ((0, 1, 8, 8, 1, 1, 0), ">= 1"), ((1, 0, 8, 8, 1, 1, 0), ">= 1"), ((1, 1, 0, 8, 1, 1, 0), ">= 1"),
           ((1, 1, 8, 0, 1, 1, 0), ">= 1"), ((2, 1, 8, 8, 1, 2, 0), "keep_largest")]
    for ints, word in bad:
        with pytest.raises(ValueError, match=word):
            plan.add_generic("components", ptrs, list(ints), [0.5], "components")
        with pytest.raises(ValueError, match=word):
            C.generic("components", ptrs, list(ints), [0.5], 0)        # (immediate style: nothing launched)
        if word not in ("keep_largest", "min_size"):
            with pytest.raises(ValueError, match=word):
                C.components_scratch(*ints[:5])
            assert word in C.components_check(*ints[:5], ints[6])
    assert "min_size" in C.components_check(2, 1, 8, 8, 1, -1)
    for thr in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            plan.add_generic("components", ptrs, [2, 1, 8, 8, 1, 1, 0], [thr], "components")
    for null in range(4):                                   # prob, out, info, scratch: none may be null
        p = list(ptrs)
        p[null] = 0
        with pytest.raises(ValueError):
            plan.add_generic("components", p, [2, 1, 8, 8, 1, 1, 0], [0.5], "components")
    with pytest.raises(ValueError):
        plan.add_generic("components", ptrs[:3], [2, 1, 8, 8, 1, 1, 0], [0.5], "components")       # no scratch pointer
    with pytest.raises(ValueError):
        plan.add_generic("components", ptrs[:3] + [16388], [2, 1, 8, 8, 1, 1, 0], [0.5], "components")   # not 16-byte aligned
    with pytest.raises(ValueError):
        plan.add_generic("components", ptrs, [2, 1, 8, 8, 1, 1], [0.5], "components")              # no min_size
    assert plan.size() == n0


def test_sample_groups_cover_the_batch_within_the_cap():
    from unet_distributed_amd.runtime.executor_base import COMP_SCRATCH_CAP, components_group
    C = _C()
    assert COMP_SCRATCH_CAP == 256 << 20
    assert components_group(C, 1024, 1, 128, 128, 1) == 1024            # 128 MiB: one group
    g = components_group(C, 1024, 1, 128, 128, 3)                       # 384 MiB: two groups of 512
    assert g == 512 and C.components_scratch(g, 1, 128, 128, 3) <= COMP_SCRATCH_CAP
    assert components_group(C, 8, 128, 128, 128, 1) == 8
    one = C.components_scratch(1, 1, 16, 24, 2)
    assert components_group(C, 5, 1, 16, 24, 2, cap=2 * one) == 2 and components_group(C, 5, 1, 16, 24, 2, cap=4 * one) == 3
    assert components_group(C, 5, 1, 16, 24, 2, cap=0) == 1             # (a cap below one sample: one sample)
    with pytest.raises(ValueError, match="classes"):
        components_group(C, 5, 1, 16, 24, 7)


ENGINES = [
    dict(out_channels=3, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp16", norm="group"),
    dict(out_channels=2, batch_size=2, img_size=16, in_channels=4, dims=3),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp32"),
]


def _dry_engine(cfg, **kw):
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.f32_engine import NativeUNetF32
    from unet_distributed_amd.runtime.native_engine import NativeUNet
    from unet_distributed_amd.runtime.params import FlatParams
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device="cpu")
    if cfg.dtype == "fp32":
        return NativeUNetF32(spec, flat, cfg.batch_size, cfg.img_size, "cpu", dry_run=True, **kw)
    return NativeUNet(spec, flat, cfg.batch_size, cfg.img_size, "cpu", dry_run=True, dtype=cfg.dtype, **kw)


@pytest.mark.parametrize("kw", ENGINES, ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_dry_run_engines_expose_components_to_plan_check(kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.runtime.plan_check import (check_components_plan, check_engine, check_stats_plan,
                                                         components_scratch)
    cfg = Config(**kw)
    off = _dry_engine(cfg)
    e = _dry_engine(cfg, eval_components=True)
    # off by default: nothing allocated, and the finding says so
    assert off.components_plan is None and off.prob_pp is None and off.components_info is None
    assert off.components_scratch is None
    assert check_components_plan(off) != []
    assert e.components_plan.names() == ["components"]
    assert check_components_plan(e) == []
    # the existing plans and buffers are what they are without the option
    assert e.stats_plan.names() == ["case_stats"] and check_stats_plan(e) == []
    assert e.plan.names() == off.plan.names() and e.eval_plan.names() == off.eval_plan.names()
    assert all("components" not in n for n in (e.plan.names(), e.eval_plan.names()))
    assert check_engine(e) == {"train": [], "eval": []}
    assert e._case_stats_args[0][0] == e.prob.data_ptr()
    B, K = cfg.batch_size, cfg.out_channels
    d = cfg.img_size if cfg.dims == 3 else 1
    assert e.prob_pp.shape == e.prob.shape and e.prob_pp.dtype == torch.float32
    assert e.prob_pp.data_ptr() != e.prob.data_ptr()
    assert e.components_info.shape == (B, K, 4) and e.components_info.dtype == torch.int32
    assert e.components_scratch.numel() * 4 == components_scratch(B, d, cfg.img_size, cfg.img_size, K)
    with pytest.raises(RuntimeError):
        e.components(0.5, True, 0)                              # validated, never launched
    # an extent past any of the three buffers is a named finding
    pp, info, scratch = e.prob_pp, e.components_info, e.components_scratch
    e.prob_pp = pp.view(-1)[:-1]
    errs = check_components_plan(e)
    assert errs and "components" in errs[0] and "past its end" in errs[0] and any("prob_pp holds" in s for s in errs)
    e.prob_pp, e.components_info = pp, info.view(-1)[:-1]
    errs = check_components_plan(e)
    assert errs and "past its end" in errs[0] and any("components_info" in s for s in errs)
    e.components_info, e.components_scratch = info, scratch[:-1]
    errs = check_components_plan(e)
    assert errs and "past its end" in errs[0] and any("components_scratch" in s for s in errs)
    e.components_scratch = scratch
    assert check_components_plan(e) == []


# ------------------------------------------------------------------ ATen backend and trainer
def _trainer_cfg(tmp, K, **kw):
    from unet_distributed_amd.config import Config
    base = dict(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                out_channels=K, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False, eval_hd95=True,
                log_jsonl=os.path.join(str(tmp), "m.jsonl"))
    return Config(**dict(base, **kw))


def _plant(tr, K):
    """Make the trainer's test set and model a known case: every target is a 6 x 6 square, the
    prediction is the target plus a 3 x 3 speck in the far corner (the 'model' reads both from
    the input channels), so the unfiltered HD95 is the distance to the speck."""
    n = len(tr.x_test)
    y = np.zeros((n, 32, 32, K), dtype=np.float32)
    x = np.full((n, 32, 32, 4), -1.0, dtype=np.float32)
    for i in range(n):
        for k in range(K):
            r, c = 2 + (i + k) % 5, 3 + (2 * i + k) % 4
            y[i, r:r + 6, c:c + 6, k] = 1
            x[i, r:r + 6, c:c + 6, k] = 1
            x[i, 29:32, 29:32, k] = 1                    # the speck
    tr.x_test, tr.y_test = x, y
    tr.backend._forward_logits = lambda params, xb, train, seed, dropout: 6.0 * xb.to(tr.device)[..., :K]


def test_cpu_trainer_scores_the_filtered_map(tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.runtime.trainer import Trainer
    from unet_distributed_amd.utils import events
    from unet_distributed_amd.utils.metrics import MetricLogger
    K = 2
    for sub in ("off", "on"):
        os.mkdir(tmp_path / sub)
    off = Trainer(_trainer_cfg(tmp_path / "off", K))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr = Trainer(_trainer_cfg(tmp_path / "on", K, eval_components="largest,min:20"))
    assert "Evaluation components: largest, min 20 voxels" in out.getvalue().split("\n")
    _plant(off, K)
    _plant(tr, K)
    m0, m = off.evaluate(), tr.evaluate()
    assert set(m) - set(m0) == {"components"} and m["components"] == "largest,min:20"
    assert set(m["per_class"]) - set(m0["per_class"]) == {"components", "components_kept"}
    # the pooled TEST DATASET block does not see the filter
    for k in ("loss", "dice", "sensitivity", "specificity", "batches"):
        assert m[k] == m0[k], k
    assert m["cases"] == m0["cases"] == 10
    # the speck: two components before the filter, one after; HD95 far without the option, 0 with it
    assert m["per_class"]["components"] == [2.0] * K and m["per_class"]["components_kept"] == [1.0] * K
    assert all(v > 20 for v in m0["per_class"]["hd95"]) and m0["hd95"] > 20
    assert m["per_class"]["hd95"] == [0.0] * K and m["hd95"] == 0.0
    assert m["per_class"]["case_dice"] == [1.0] * K and all(v < 1.0 for v in m0["per_class"]["case_dice"])
    # the per-class soft Dice is of the filtered map
    assert all(a > b for a, b in zip(m["per_class"]["dice"], m0["per_class"]["dice"]))
    # the eval methods one by one
    x, y = torch.from_numpy(tr.x_test[:3]), torch.from_numpy(tr.y_test[:3])
    info = tr.backend.eval_components(x, y, 0.5)
    assert info.tolist() == [[[2, 1, 36, 36]] * K] * 3
    raw = off.backend.predict(x)
    want = components_torch(raw, 0.5, True, 20)[0]
    assert torch.equal(tr.backend.predict(x), want) and not torch.equal(raw, want)
    assert torch.equal(tr.backend.eval_stats(x, y, 0.5), seg_metrics.case_stats_torch(want, y, 0.5))
    assert torch.equal(tr.backend.eval_surface(x, y, 0.5), seg_metrics.case_surface_torch(want, y, 0.5))
    assert torch.equal(tr.backend.eval_sums(x, y), off.backend.eval_sums(x, y))
    assert torch.equal(tr.backend.last_eval_components(0.5), info)
    with pytest.raises(RuntimeError, match="eval_components"):
        off.backend.eval_components(x, y, 0.5)
    # the report: the new field on each per-class line, JSONL and TensorBoard keys
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr.log.test(3, m, 1, 1, final=True)
        off.log.test(3, m0, 1, 1, final=True)
    tr.log.close()
    off.log.close()
    lines = out.getvalue().split("\n")
    for k in range(K):
        assert lines[6 + k].startswith("class %d: Dice = " % k) and lines[6 + k].endswith(", components = 2.00 -> 1.00")
    assert "components" not in "\n".join(lines[7 + 2 * K + 1:])             # the report with the option off
    rec = json.loads(open(tr.cfg.log_jsonl).read().strip().split("\n")[-1])
    assert rec["components"] == "largest,min:20" and rec["per_class"]["components"] == [2.0] * K
    assert rec["per_class"]["components_kept"] == [1.0] * K
    assert "components" not in open(off.cfg.log_jsonl).read()
    tb = MetricLogger(Config(tensorboard=True, progress=False), True, str(tmp_path / "tb"))
    with contextlib.redirect_stdout(io.StringIO()):
        tb.test(3, m, 1, 1)
    path = tb.events.path
    tb.close()
    tags = {}
    for step, r in events.read_events(path):
        tags.update({k: v for k, v in r.items() if v is not None})
    for k in range(K):
        assert tags["components_test/class_%d" % k] == 2.0 and tags["components_kept_test/class_%d" % k] == 1.0


def test_report_without_the_option_is_unchanged(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr = Trainer(_trainer_cfg(tmp_path, 2, eval_hd95=False))
    assert "components" not in out.getvalue()
    assert tr.backend.components is None
    m = tr.evaluate()
    assert set(m) == {"loss", "dice", "sensitivity", "specificity", "batches", "per_class", "case_dice", "cases"}
    assert set(m["per_class"]) == {"dice", "case_dice", "sensitivity", "specificity"}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr.log.test(3, m, 1, 1)
    tr.log.close()
    assert "components" not in out.getvalue() and "components" not in open(tr.cfg.log_jsonl).read()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    torch.set_num_threads(2)
    from unet_distributed_amd.parallel import dist as D
    from unet_distributed_amd.runtime.trainer import Trainer
    cfg = _trainer_cfg(os.path.join(out, "r%d" % rank), 3, batch_size=8, dist_backend="gloo", dist_timeout_s=120.0,
                       eval_components="min:3")
    cfg.log_jsonl = ""
    tr = Trainer(cfg)                       # per-rank batch 4, 10 test cases: 2 full batches + a tail of 2
    m = tr.evaluate()
    with open(os.path.join(out, "r%d.json" % rank), "w") as f:
        json.dump(seg_metrics.jsonable(m), f)
    D.destroy()


def test_two_ranks_report_the_one_rank_components(tmp_path):
    """The component sums are allreduced with the other accumulators (HD95 sits between them)."""
    from unet_distributed_amd.runtime.trainer import Trainer
    mp.spawn(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (json.load(open(tmp_path / ("r%d.json" % r))) for r in range(2))
    assert a == b
    one = Trainer(_trainer_cfg(tmp_path / "one", 3, log_jsonl="", eval_components="min:3")).evaluate()
    assert a["per_class"]["components"] == one["per_class"]["components"]
    assert a["per_class"]["components_kept"] == one["per_class"]["components_kept"]
    assert np.allclose(a["per_class"]["hd95"], one["per_class"]["hd95"], rtol=0, atol=1e-12)
    assert a["components"] == "min:3" and a["cases"] == 10


def test_tta_filters_the_mean_and_sliding_the_blended_map(tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import TorchBackend
    from unet_distributed_amd.runtime.params import FlatParams
    kw = dict(img_size=16, in_channels=4, out_channels=2, dtype="fp32", eval_tta="flip")
    spec = spec_from_config(Config(**kw))
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    off = TorchBackend(spec, flat, Config(**kw), "cpu", 2)
    on = TorchBackend(spec, flat, Config(eval_components="largest", **kw), "cpu", 2)
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.randn(2, 16, 16, 4).astype(np.float32))
    assert torch.equal(on.predict(x), components_torch(off.predict(x), 0.5, True, 0)[0])
    big = torch.from_numpy(rng.randn(1, 20, 28, 4).astype(np.float32))
    y = torch.from_numpy((rng.rand(1, 20, 28, 2) < 0.3).astype(np.float32))
    raw = off.predict_sliding(big)
    want, info = components_torch(raw, 0.5, True, 0)
    p = on.predict_sliding(big)
    assert torch.equal(p, want) and torch.equal(on.sliding_components(p, 0.5), info)
    assert torch.equal(on.sliding_stats(p, y, 0.5), seg_metrics.case_stats_torch(want, y, 0.5))
    assert torch.equal(on.sliding_surface(raw, y, 0.5), seg_metrics.case_surface_torch(want, y, 0.5))


# ------------------------------------------------------------------ inference
def _export(tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    return export_model(cfg, spec, flat)


def test_predictor_components_on_the_aten_path(tmp_path):
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    d = _export(tmp_path)
    plain = load_saved_model(d, device="cpu", batch=4, backend="torch")
    model = load_saved_model(d, device="cpu", batch=4, backend="torch", components="largest,min:3")
    with pytest.raises(SystemExit):
        load_saved_model(d, device="cpu", batch=4, backend="torch", components="tiny")
    x, y = synthetic_brats(6, 32, 4, 2, seed=1, out_channels=3)
    want, info = components_torch(torch.from_numpy(plain.predict(x)), 0.5, True, 3)
    assert np.array_equal(model.predict(x), want.numpy())
    got = model.components(x)
    assert got.shape == (6, 3, 4) and got.dtype == np.int64 and np.array_equal(got, info.numpy())
    yt = torch.from_numpy(y).float()
    assert np.array_equal(model.surface(x, y), seg_metrics.case_surface_torch(want, yt, 0.5).numpy())
    assert np.array_equal(model.stats(x, y), seg_metrics.case_stats_torch(want, yt, 0.5).numpy())
    rng = np.random.RandomState(4)
    big = rng.randn(2, 40, 56, 4).astype(np.float32)
    want, info = components_torch(torch.from_numpy(plain.predict_sliding(big)), 0.5, True, 3)
    assert np.array_equal(model.predict_sliding(big), want.numpy())
    assert np.array_equal(model.components_sliding(big), info.numpy())
    with pytest.raises(RuntimeError, match="components"):
        plain.components(x)


def test_sanity_check_components_lines(tmp_path):
    from unet_distributed_amd import sanity_check
    d = _export(tmp_path)
    argv = ["--export_dir", d, "--batch_size", "4", "--synthetic", "10", "--device", "cpu", "--backend", "torch"]

    def run(extra):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            sanity_check.main(argv + extra)
        return out.getvalue().split("\n")

    plain = run(["--per_class", "--hd95"])
    on = run(["--per_class", "--hd95", "--components", "largest"])
    assert not any("components = " in l or "Evaluation components" in l for l in plain)
    assert on[1] == "Evaluation components: largest" and on[0] == plain[0] and on[2:5] == plain[1:4]
    cls = [l for l in on if l.startswith("class ") and "case Dice" in l]
    assert len(cls) == 3 and all(", components = " in l and " -> " in l for l in cls)
    assert any(l.startswith("HD95 = ") for l in on)
    sw = run(["--per_class", "--hd95", "--components", "largest,min:2", "--sliding", "--synthetic_size", "40"])
    assert sw[1] == "Evaluation components: largest, min 2 voxels"
    assert len([l for l in sw if ", components = " in l]) == 3
    with pytest.raises(SystemExit):
        run(["--components", "smallest"])

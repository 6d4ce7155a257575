"""95th-percentile Hausdorff distance off the GPU: the all-pairs oracle and the host maths
(ops/seg_metrics.py) on hand cases and against scipy, plan-time validation of the surf_dist
op on the CPU dry run, dry-run executors with --eval_hd95, and the trainer's report on the
ATen backend (one and two ranks)."""
import contextlib
import io
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from unet_distributed_amd.ops import seg_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _surf(p, t, thr=0.5):
    """Oracle integers of one boolean / float mask pair on its own grid, K = 1."""
    p = torch.as_tensor(np.asarray(p, dtype=np.float32))[None, ..., None]
    t = torch.as_tensor(np.asarray(t, dtype=np.float32))[None, ..., None]
    return seg_metrics.case_surface_torch(p, t, thr)


# ------------------------------------------------------------------ hand cases
def test_two_single_voxels():
    p, t = np.zeros((5, 6)), np.zeros((5, 6))
    p[0, 0] = 1
    t[3, 4] = 1
    s = _surf(p, t)
    assert s.dtype == torch.int64 and s.shape == (1, 1, 4)
    assert s[0, 0].tolist() == [1, 1, 25, 25]
    assert seg_metrics.hd95_from_surface(s, (5, 6))[0, 0] == 5.0


def test_equal_masks_have_zero_distances():
    rng = np.random.RandomState(0)
    p = rng.rand(9, 11) < 0.4
    s = _surf(p, p)
    assert s[0, 0, 0] == s[0, 0, 1] > 0 and s[0, 0, 2:].tolist() == [0, 0]
    assert seg_metrics.hd95_from_surface(s, (9, 11))[0, 0] == 0.0


@pytest.mark.parametrize("grid", [(6, 8), (4, 6, 8)])
def test_empty_case_rules(grid):
    z, one = np.zeros(grid), np.zeros(grid)
    one[(1,) * len(grid)] = 1
    diag = math.sqrt(sum(v * v for v in grid) + (1 if len(grid) == 2 else 0))     # D = 1 in 2D
    assert _surf(z, z)[0, 0].tolist() == [0, 0, -1, -1]
    assert seg_metrics.hd95_from_surface(_surf(z, z), grid)[0, 0] == 0.0
    assert _surf(one, z)[0, 0].tolist() == [1, 0, -1, -1]
    assert seg_metrics.hd95_from_surface(_surf(one, z), grid)[0, 0] == diag
    assert _surf(z, one)[0, 0].tolist() == [0, 1, -1, -1]
    assert seg_metrics.hd95_from_surface(_surf(z, one), grid)[0, 0] == diag
    if len(grid) == 2:                       # (a one-slice volume is the 2D grid)
        assert seg_metrics.hd95_from_surface(_surf(one, z), (1,) + grid)[0, 0] == diag
        assert seg_metrics.hd95_from_surface(_surf(z, one), (240, 240, 155))[0, 0] == pytest.approx(373.13, abs=5e-3)


@pytest.mark.parametrize("grid", [(5, 7), (4, 5, 6)])
def test_full_foreground_surface_is_the_border(grid):
    full = np.ones(grid)
    border = int(np.prod(grid) - np.prod([v - 2 for v in grid]))
    s = _surf(full, full)
    assert s[0, 0].tolist() == [border, border, 0, 0]


def test_threshold_is_inclusive_in_fp32_and_classes_are_separate():
    p = np.zeros((2, 4, 6, 2), dtype=np.float32)
    t = np.zeros((2, 4, 6, 2), dtype=np.float32)
    p[0, 1, 1, 0] = np.float32(0.3)          # exactly at the threshold: foreground
    p[0, 1, 2, 0] = np.nextafter(np.float32(0.3), np.float32(0))
    t[0, 1, 4, 0] = 1.0
    p[1, 0, 0, 1] = 0.9
    t[1, 3, 5, 1] = 0.5                      # t >= 0.5 is foreground
    s = seg_metrics.case_surface_torch(torch.from_numpy(p), torch.from_numpy(t), 0.3)
    assert s[0, 0].tolist() == [1, 1, 9, 9] and s[1, 1].tolist() == [1, 1, 34, 34]
    assert s[0, 1].tolist() == [0, 0, -1, -1] and s[1, 0].tolist() == [0, 0, -1, -1]
    flat = seg_metrics.case_surface_torch(torch.from_numpy(p).view(2, 24, 2), torch.from_numpy(t).view(2, 24, 2), 0.3,
                                          grid=(1, 4, 6))
    assert torch.equal(flat, s)


def test_rank_interpolation():
    # m = 2: r = 95, lo = 0, hi = 1 -> sqrt(q_lo) + 0.95 (sqrt(q_hi) - sqrt(q_lo))
    h = seg_metrics.hd95_from_surface(np.array([[[1, 1, 4, 9]]]), (8, 8))
    assert h[0, 0] == 2.0 + 95 / 100.0 * (3.0 - 2.0)
    # m = 41: r = 3800, no fraction
    h = seg_metrics.hd95_from_surface(np.array([[[20, 21, 16, 25]]]), (8, 8))
    assert h[0, 0] == 4.0


def _blobs(rng, grid, seeds):
    """Random blobs: a few seeds dilated by a random number of face-neighbour steps."""
    m = np.zeros(grid, dtype=bool)
    for _ in range(seeds):
        m[tuple(rng.randint(0, v) for v in grid)] = True
    for _ in range(rng.randint(1, 4)):
        g = m.copy()
        for ax in range(m.ndim):
            g |= np.roll(m, 1, ax) | np.roll(m, -1, ax)
        m = g & (rng.rand(*grid) < 0.9)
    return m


@pytest.mark.parametrize("grid", [(8, 8), (16, 24), (7, 9, 8), (32, 32)])
def test_scipy_cross_check(grid):
    """hd95_from_surface(case_surface_torch) against the distance-transform formulation: 1e-9
    covers float64 rounding of values below 1000."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(sum(grid))
    done = 0
    for trial in range(12):
        p, t = _blobs(rng, grid, 3), _blobs(rng, grid, 3)
        sp, st = p & ~ndi.binary_erosion(p), t & ~ndi.binary_erosion(t)
        if not sp.any() or not st.any():
            continue
        want = np.percentile(np.hstack([ndi.distance_transform_edt(~st)[sp], ndi.distance_transform_edt(~sp)[st]]), 95)
        s = _surf(p, t)
        assert s[0, 0, 0] == sp.sum() and s[0, 0, 1] == st.sum()
        got = seg_metrics.hd95_from_surface(s, grid)[0, 0]
        print("hd95 vs scipy", grid, trial, abs(got - want))
        assert abs(got - want) <= 1e-9, (grid, trial, got, want)
        done += 1
    assert done >= 6


def test_accumulators_of_disjoint_case_sets_add():
    surf = np.array([[[1, 1, 25, 25], [0, 0, -1, -1]], [[3, 0, -1, -1], [2, 2, 1, 4]], [[5, 6, 9, 16], [0, 4, -1, -1]]])
    grid = (6, 8)
    a, b, ab = (seg_metrics.accumulate_hd95(s, grid) for s in (surf[:1], surf[1:], surf))
    for k in a:
        assert np.array_equal(np.asarray(a[k]) + np.asarray(b[k]), np.asarray(ab[k]))
    assert ab["cases"] == 3.0
    m = seg_metrics.hd95_metrics(ab)
    assert m["hd95"] == pytest.approx(list(seg_metrics.hd95_from_surface(surf, grid).mean(0)))
    assert m["hd95_mean"] == pytest.approx(np.mean(m["hd95"]))
    one = seg_metrics.accumulate_hd95(surf, grid, valid=[True, False, True])
    assert one["cases"] == 2.0 and one["hd95_sum"][0] == 5.0 + seg_metrics.hd95_from_surface(surf[2:], grid)[0, 0]


def test_eval_hd95_flag_parses():
    from unet_distributed_amd.config import Config, parse_args
    assert Config().eval_hd95 is False and parse_args([]).eval_hd95 is False
    assert parse_args(["--eval_hd95"]).eval_hd95 is True
    assert parse_args(["--eval_hd95=false"]).eval_hd95 is False
    assert parse_args(["--noeval_hd95"]).eval_hd95 is False


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


GOOD = [(3, 1, 8, 8, 1), (2, 1, 16, 24, 3), (1024, 1, 128, 128, 4), (8, 128, 128, 128, 1), (1, 1, 8, 512, 2),
        (1, 155, 240, 240, 3)]


@pytest.mark.parametrize("kind", ["surf_dist", "f32_surf_dist"])
def test_surf_dist_plan_time_validation(kind):
    from unet_distributed_amd.runtime.plan_check import surf_dist_scratch
    C = _C()
    plan = C.Plan(0)
    ptrs = [4096, 8192, 12288, 16384]
    for shape in GOOD:
        i = plan.add_generic(kind, ptrs, list(shape), [0.5], "case_surface")
        assert plan.check_dispatch(i, i + 1) == []
        assert surf_dist_scratch(*shape) == C.surf_dist_scratch(*shape) == shape[0] * shape[4] * 2 * 4 * int(
            np.prod(shape[1:4]))
    n0 = plan.size()
    bad = [(2, 1, 8, 8, 0), (2, 1, 8, 8, 5),            # K outside 1..4
           (2, 1, 6, 6, 1), (1, 3, 3, 3, 1),            # S % 8
           (1, 256, 256, 256, 1),                       # S = 2^24
           (1 << 10, 1, 1024, 1024, 2),                 # N S K = 2^31
           (0, 1, 8, 8, 1), (1, 0, 8, 8, 1), (1, 1, 0, 8, 1), (1, 1, 8, 0, 1)]
    for shape in bad:
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, list(shape), [0.5], "case_surface")
        with pytest.raises(ValueError):
            C.generic(kind, ptrs, list(shape), [0.5], 0)                # (immediate style: nothing launched)
        with pytest.raises(ValueError):
            C.surf_dist_scratch(*shape)
    for null in range(4):                               # prob, target, output, scratch: none may be null
        p = list(ptrs)
        p[null] = 0
        with pytest.raises(ValueError):
            plan.add_generic(kind, p, [2, 1, 8, 8, 1], [0.5], "case_surface")
    with pytest.raises(ValueError):
        plan.add_generic(kind, ptrs[:3], [2, 1, 8, 8, 1], [0.5], "case_surface")        # no scratch pointer
    with pytest.raises(ValueError):
        plan.add_generic(kind, ptrs[:3] + [16388], [2, 1, 8, 8, 1], [0.5], "case_surface")   # not 16-byte aligned
    assert plan.size() == n0


def test_sample_groups_cover_the_batch_within_the_scratch():
    from unet_distributed_amd.runtime.executor_base import SURF_SCRATCH_CAP, surf_dist_group
    C = _C()
    assert SURF_SCRATCH_CAP == 256 << 20
    one = C.surf_dist_scratch(1, 1, 128, 128, 4)
    g = surf_dist_group(1024, one, SURF_SCRATCH_CAP)
    assert g == 512 and C.surf_dist_scratch(g, 1, 128, 128, 4) <= SURF_SCRATCH_CAP
    assert surf_dist_group(8, C.surf_dist_scratch(1, 128, 128, 128, 1), SURF_SCRATCH_CAP) == 8
    # K = 3: 682 samples fit, two groups of 512 cover the batch; five samples through room for two: 2 + 2 + 1
    assert surf_dist_group(1024, C.surf_dist_scratch(1, 1, 128, 128, 3), SURF_SCRATCH_CAP) == 512
    assert surf_dist_group(5, one, 2 * one) == 2 and surf_dist_group(5, one, 4 * one) == 3
    with pytest.raises(ValueError):
        surf_dist_group(4, one, one - 1)


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
def test_dry_run_engines_expose_case_surface_to_plan_check(kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.runtime.plan_check import (check_engine, check_stats_plan, check_surface_plan,
                                                         surf_dist_scratch)
    cfg = Config(eval_hd95=True, **kw)
    off = _dry_engine(cfg)
    e = _dry_engine(cfg, eval_hd95=True)
    # off by default: nothing allocated, and the finding says so
    assert off.surface_plan is None and off.case_surface_buf is None and off.case_surface_scratch is None
    assert check_surface_plan(off) != []
    assert e.surface_plan.names() == ["case_surface"]
    assert check_surface_plan(e) == []
    # the existing plans are what they are without the flag
    assert e.stats_plan.names() == ["case_stats"] and check_stats_plan(e) == []
    assert e.plan.names() == off.plan.names() and e.eval_plan.names() == off.eval_plan.names()
    assert all("case_surface" not in n for n in (e.plan.names(), e.eval_plan.names()))
    assert check_engine(e) == {"train": [], "eval": []}
    B, K = cfg.batch_size, cfg.out_channels
    d = cfg.img_size if cfg.dims == 3 else 1
    assert e.case_surface_buf.shape == (B, K, 4) and e.case_surface_buf.dtype == torch.int32
    assert e.case_surface_scratch.numel() * 4 == surf_dist_scratch(B, d, cfg.img_size, cfg.img_size, K)
    with pytest.raises(RuntimeError):
        e.case_surface()                                        # validated, never launched
    # an extent past either buffer is a named finding
    buf, scratch = e.case_surface_buf, e.case_surface_scratch
    e.case_surface_buf = buf.view(-1)[:-1]
    errs = check_surface_plan(e)
    assert errs and "case_surface" in errs[0] and "past its end" in errs[0]
    e.case_surface_buf, e.case_surface_scratch = buf, scratch[:-1]
    errs = check_surface_plan(e)
    assert errs and "case_surface" in errs[0] and "past its end" in errs[0]
    assert any("case_surface_scratch" in s for s in errs)
    e.case_surface_scratch = scratch
    assert check_surface_plan(e) == []


# ------------------------------------------------------------------ trainer on the ATen backend
def _trainer_cfg(tmp, K, **kw):
    from unet_distributed_amd.config import Config
    base = dict(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                out_channels=K, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False, eval_hd95=True,
                log_jsonl=os.path.join(str(tmp), "m.jsonl"))
    return Config(**dict(base, **kw))


def test_cpu_trainer_reports_hd95_over_every_case(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.utils import events
    from unet_distributed_amd.utils.metrics import MetricLogger
    K = 3
    cfg = _trainer_cfg(tmp_path, K)
    tr = Trainer(cfg)
    m = tr.evaluate()
    assert m["batches"] == 2 and m["cases"] == 10 == len(tr.x_test)          # two full batches and a tail of 2
    surf = seg_metrics.case_surface_torch(tr.backend.predict(torch.from_numpy(tr.x_test)),
                                          torch.from_numpy(tr.y_test), cfg.eval_threshold)
    want = seg_metrics.hd95_from_surface(surf, (32, 32)).mean(0)
    assert set(m["per_class"]) == {"dice", "case_dice", "sensitivity", "specificity", "hd95"}
    assert len(m["per_class"]["hd95"]) == K
    assert np.allclose(m["per_class"]["hd95"], want, rtol=0, atol=1e-9), (m["per_class"]["hd95"], want)
    assert abs(m["hd95"] - want.mean()) <= 1e-9
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr.log.test(3, m, 1, 1, final=True)
    tr.log.close()
    lines = out.getvalue().split("\n")
    assert lines[6 + K].startswith("Case Dice = ")                            # the existing block, then the new lines
    assert lines[7 + K:7 + 2 * K] == ["class %d: HD95 = %s" % (k, seg_metrics.fmt(m["per_class"]["hd95"][k]))
                                      for k in range(K)]
    assert lines[7 + 2 * K] == "HD95 = %s (10 cases)" % seg_metrics.fmt(m["hd95"])
    rec = json.loads(open(cfg.log_jsonl).read().strip().split("\n")[-1])
    assert rec["kind"] == "test_final" and rec["hd95"] == m["hd95"] and rec["per_class"]["hd95"] == m["per_class"]["hd95"]
    # TensorBoard: the report of this evaluation through an event-writing logger
    tb = MetricLogger(Config(tensorboard=True, progress=False), True, str(tmp_path / "tb"))
    assert tb.events is not None
    with contextlib.redirect_stdout(io.StringIO()):
        tb.test(3, m, 1, 1)
    path = tb.events.path
    tb.close()
    tags = {}
    for step, r in events.read_events(path):
        tags.update({k: v for k, v in r.items() if v is not None})
    assert abs(tags["hd95_test"] - m["hd95"]) <= 1e-5 * max(1.0, m["hd95"])
    for k in range(K):
        assert abs(tags["hd95_test/class_%d" % k] - m["per_class"]["hd95"][k]) <= 1e-5 * max(1.0, m["per_class"]["hd95"][k])


def test_report_without_the_flag_is_unchanged(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    tr = Trainer(_trainer_cfg(tmp_path, 2, eval_hd95=False))
    m = tr.evaluate()
    assert set(m) == {"loss", "dice", "sensitivity", "specificity", "batches", "per_class", "case_dice", "cases"}
    assert set(m["per_class"]) == {"dice", "case_dice", "sensitivity", "specificity"}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr.log.test(3, m, 1, 1)
    tr.log.close()
    assert "HD95" not in out.getvalue() and "hd95" not in open(tr.cfg.log_jsonl).read()


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
    cfg = _trainer_cfg(os.path.join(out, "r%d" % rank), 3, batch_size=8, dist_backend="gloo", dist_timeout_s=120.0)
    cfg.log_jsonl = ""
    tr = Trainer(cfg)                       # per-rank batch 4, 10 test cases: 2 full batches + a tail of 2
    m = tr.evaluate()
    with open(os.path.join(out, "r%d.json" % rank), "w") as f:
        json.dump(seg_metrics.jsonable(m), f)
    D.destroy()


def test_two_ranks_report_the_one_rank_hd95(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    mp.spawn(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (json.load(open(tmp_path / ("r%d.json" % r))) for r in range(2))
    assert a == b
    one = Trainer(_trainer_cfg(tmp_path / "one", 3, log_jsonl="")).evaluate()
    assert np.allclose(a["per_class"]["hd95"], one["per_class"]["hd95"], rtol=0, atol=1e-12)
    assert abs(a["hd95"] - one["hd95"]) <= 1e-12


def test_sanity_check_hd95_lines(tmp_path):
    from unet_distributed_amd import sanity_check
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    d = export_model(cfg, spec, flat)
    argv = ["--export_dir", d, "--batch_size", "4", "--synthetic", "10", "--device", "cpu", "--backend", "torch"]

    def run(extra):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            sanity_check.main(argv + extra)
        return out.getvalue().split("\n")

    plain, per = run([]), run(["--hd95"])
    assert per[:5] == plain[:5] and not any("HD95" in l for l in plain)
    model = load_saved_model(d, device="cpu", batch=4, backend="torch")
    x, y = synthetic_brats(10, 32, 4, 2, seed=1, out_channels=3)
    surf = model.surface(x[:8], y[:8])
    assert surf.shape == (8, 3, 4) and surf.dtype == np.int64
    want = seg_metrics.case_surface_torch(torch.from_numpy(model.predict(x[:8])), torch.from_numpy(y[:8]).float(), 0.5)
    assert np.array_equal(surf, want.numpy())
    h = seg_metrics.hd95_from_surface(surf, (32, 32)).mean(0)
    for k in range(3):
        assert per[5 + k] == "class {}: HD95 = {}".format(k, seg_metrics.fmt(h[k]))
    assert per[8] == "HD95 = {} (8 cases)".format(seg_metrics.fmt(h.mean()))
    assert per[9].startswith("(2 batches, torch backend, ")

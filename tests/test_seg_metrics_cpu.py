"""Per-class / per-case evaluation metrics off the GPU: the torch oracle and the metric maths
(ops/seg_metrics.py), plan-time validation of the seg_stats op on the CPU dry run, the
trainer's evaluation report on the ATen backend (one and two ranks), the --eval_threshold
flag and sanity_check --per_class."""
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


# ------------------------------------------------------------------ oracle and metric maths
def _brute(prob, target, thr):
    N, S, K = prob.shape
    out = np.zeros((N, K, 6))
    thr32 = np.float32(thr)
    for n in range(N):
        for s in range(S):
            for k in range(K):
                p, t = prob[n, s, k], target[n, s, k]
                out[n, k, 0] += float(t) * float(p)
                out[n, k, 1] += float(t)
                out[n, k, 2] += float(p)
                pos, fg = p >= thr32, t >= 0.5
                out[n, k, 3] += pos and fg
                out[n, k, 4] += pos and not fg
                out[n, k, 5] += (not pos) and fg
    return out


@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_torch_oracle_equals_a_brute_force_loop(thr):
    rng = np.random.RandomState(3)
    prob = rng.rand(3, 40, 3).astype(np.float32)
    prob[rng.rand(3, 40, 3) < 0.2] = np.float32(thr)          # the >= side counts as positive
    target = (rng.rand(3, 40, 3) > 0.5).astype(np.float32)
    got = seg_metrics.case_stats_torch(torch.from_numpy(prob).view(3, 5, 8, 3), torch.from_numpy(target).view(3, 5, 8, 3),
                                       thr)
    want = _brute(prob, target, thr)
    assert got.dtype == torch.float64 and got.shape == (3, 3, 6)
    assert np.array_equal(got[..., 3:].numpy(), want[..., 3:])
    assert np.allclose(got[..., :3].numpy(), want[..., :3], rtol=1e-13, atol=0)
    at = prob == np.float32(thr)
    assert at.any() and want[..., 3].sum() + want[..., 4].sum() >= at.sum()


def test_metric_definitions_and_the_empty_case_convention():
    S = 100
    #        I    St   Sp   TP  FP  FN
    stats = np.array([[[8.0, 10.0, 12.0, 8, 2, 2], [0.0, 0.0, 0.5, 0, 0, 0]],      # class 1: empty target, empty prediction
                      [[3.0, 5.0, 4.0, 3, 1, 2], [0.0, 0.0, 3.0, 0, 4, 0]]])       # class 1: empty target, 4 false positives
    m = seg_metrics.metrics_from_case_stats(stats, S)
    assert m["cases"] == 2
    assert m["dice"] == pytest.approx([(2 * 11 + 1) / (15 + 16 + 1), 1.0 / (0 + 3.5 + 1)])
    assert m["case_dice"] == pytest.approx([(16 / 20 + 6 / 9) / 2, (1.0 + 0.0) / 2])
    assert m["case_dice_mean"] == pytest.approx(np.mean(m["case_dice"]))
    assert m["sensitivity"][0] == pytest.approx(11 / 15) and math.isnan(m["sensitivity"][1])   # TP + FN == 0
    assert m["specificity"] == pytest.approx([(200 - 11 - 3 - 4) / (200 - 11 - 4), (200 - 4) / 200])
    one = seg_metrics.metrics_from_case_stats(stats, S, valid=[True, False])
    assert one["cases"] == 1 and one["case_dice"] == pytest.approx([0.8, 1.0])
    # accumulators of disjoint case sets add
    a, b, ab = (seg_metrics.accumulate(s, S) for s in (stats[:1], stats[1:], stats))
    for k in a:
        assert np.allclose(np.asarray(a[k]) + np.asarray(b[k]), ab[k])
    # every pixel a true positive: no negatives -> specificity undefined
    full = seg_metrics.metrics_from_case_stats(np.array([[[100.0, 100.0, 100.0, 100, 0, 0]]]), S)
    assert math.isnan(full["specificity"][0]) and full["sensitivity"] == [1.0]


def test_nan_is_logged_as_json_null(tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.utils.metrics import MetricLogger
    rec = seg_metrics.jsonable({"a": float("nan"), "b": [1.0, float("inf"), np.float64("nan")], "c": {"d": 2, "e": "x"}})
    assert rec == {"a": None, "b": [1.0, None, None], "c": {"d": 2, "e": "x"}}
    path = tmp_path / "m.jsonl"
    log = MetricLogger(Config(log_jsonl=str(path), tensorboard=False), True, str(tmp_path))
    m = {"loss": 0.5, "dice": 0.25, "sensitivity": 0.75, "specificity": 0.125, "batches": 1,
         "per_class": {"dice": [0.25], "case_dice": [1.0], "sensitivity": [float("nan")], "specificity": [0.5]},
         "case_dice": 1.0, "cases": 3}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        log.test(7, m, 1, 2)
    log.close()
    text = path.read_text()
    assert "NaN" not in text
    rec = json.loads(text)
    assert rec["per_class"]["sensitivity"] == [None] and rec["cases"] == 3 and rec["kind"] == "test"
    lines = out.getvalue().split("\n")
    # the existing block, line for line, then the new lines
    assert lines[:6] == ["", "Epoch 1 of 2: TEST DATASET", "loss = 0.5000", "Dice = 0.2500", "Sensitivity = 0.7500",
                         "Specificity = 0.1250"]
    assert lines[6] == "class 0: Dice = 0.2500, case Dice = 1.0000, sensitivity = nan, specificity = 0.5000"
    assert lines[7] == "Case Dice = 1.0000 (3 cases)"


def test_tensorboard_gets_the_per_class_tags(tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.utils import events
    from unet_distributed_amd.utils.metrics import MetricLogger
    log = MetricLogger(Config(tensorboard=True, progress=False), True, str(tmp_path))
    assert log.events is not None
    m = {"loss": 0.5, "dice": 0.25, "sensitivity": 0.75, "specificity": 0.125, "batches": 1,
         "per_class": {"dice": [0.25, 0.5], "case_dice": [1.0, 0.75], "sensitivity": [0.5, 0.5],
                       "specificity": [0.5, 0.5]}, "case_dice": 0.875, "cases": 3}
    with contextlib.redirect_stdout(io.StringIO()):
        log.test(7, m, 1, 2)
    path = log.events.path
    log.close()
    tags = {}
    for step, rec in events.read_events(path):
        tags.update({k: v for k, v in rec.items() if v is not None})
    want = {"dice_test": 0.25, "dice_test/class_0": 0.25, "dice_test/class_1": 0.5, "case_dice_test/class_0": 1.0,
            "case_dice_test/class_1": 0.75, "case_dice_test": 0.875, "loss_test": 0.5}
    for k, v in want.items():
        assert abs(tags[k] - v) < 1e-6, k


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


@pytest.mark.parametrize("kind", ["seg_stats", "f32_seg_stats"])
def test_seg_stats_plan_time_validation(kind):
    from unet_distributed_amd.runtime.plan_check import seg_stats_chunks
    C = _C()
    plan = C.Plan(0)
    ptrs = [4096, 8192, 12288, 16384]
    for N, S, K in ((3, 248, 3), (1, 8, 1), (2, 262144, 4), (1024, 16384, 1), (8, 2097152, 1)):
        i = plan.add_generic(kind, ptrs, [N, S, K], [0.5], "case_stats")
        assert plan.check_dispatch(i, i + 1) == []
        assert seg_stats_chunks(N, S, K) == C.seg_stats_chunks(N, S, K)
    n0 = plan.size()
    for N, S, K in ((2, 248, 5), (2, 248, 0), (2, 252, 1), (1, 1 << 24, 1), (1 << 10, 1 << 20, 2)):
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, [N, S, K], [0.5], "case_stats")
        with pytest.raises(ValueError):
            C.generic(kind, ptrs, [N, S, K], [0.5], 0)                  # (immediate style: nothing launched)
    assert plan.size() == n0
    with pytest.raises(ValueError):
        plan.add_generic(kind, ptrs[:3], [2, 262144, 1], [0.5], "")     # split samples need the partial buffer
    plan.add_generic(kind, ptrs[:3], [3, 248, 1], [0.5], "")            # one chunk: none needed


ENGINES = [
    dict(out_channels=3, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp16", norm="group"),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, norm="batch", use_upsampling=True),
    dict(out_channels=2, batch_size=2, img_size=16, in_channels=4, dims=3),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp32"),
]


@pytest.mark.parametrize("kw", ENGINES, ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_dry_run_engines_expose_case_stats_to_plan_check(kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.f32_engine import NativeUNetF32
    from unet_distributed_amd.runtime.native_engine import NativeUNet
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.runtime.plan_check import check_engine, check_stats_plan, seg_stats_chunks
    cfg = Config(**kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device="cpu")
    if cfg.dtype == "fp32":
        e = NativeUNetF32(spec, flat, cfg.batch_size, cfg.img_size, "cpu", dry_run=True)
    else:
        e = NativeUNet(spec, flat, cfg.batch_size, cfg.img_size, "cpu", dry_run=True, dtype=cfg.dtype)
    names = (e.plan.names(), e.eval_plan.names())
    assert e.stats_plan.names() == ["case_stats"] and all("case_stats" not in n for n in names)
    assert check_stats_plan(e) == []
    assert check_engine(e) == {"train": [], "eval": []}
    B, K = cfg.batch_size, cfg.out_channels
    S = cfg.img_size ** cfg.dims
    assert e.case_stats_buf.shape == (B, K, 6)
    assert e.case_stats_partial.numel() >= B * seg_stats_chunks(B, S, K) * 6 * K
    with pytest.raises(RuntimeError):
        e.case_stats()                                          # validated, never launched
    # an extent past the buffer is a finding
    e.case_stats_buf = e.case_stats_buf.view(-1)[:-1]
    errs = check_stats_plan(e)
    assert errs and "past its end" in errs[0]


@pytest.mark.parametrize("N,S", [(1024, 128 * 128), (8, 128 ** 3)])
def test_bench_shapes_fill_the_cus(N, S):
    """The 2D and 3D bench shapes: at least 4 workgroups per CU whichever axis is long."""
    for K in (1, 3):
        assert N * _C().seg_stats_chunks(N, S, K) >= 1024


# ------------------------------------------------------------------ trainer on the ATen backend
def _trainer_cfg(tmp, K, **kw):
    from unet_distributed_amd.config import Config
    base = dict(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                out_channels=K, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False,
                log_jsonl=os.path.join(str(tmp), "m.jsonl"))
    return Config(**dict(base, **kw))


@pytest.mark.parametrize("K", [3, 1])
def test_cpu_trainer_scores_every_case(tmp_path, K):
    from unet_distributed_amd.runtime.trainer import Trainer, metrics_from_sums
    cfg = _trainer_cfg(tmp_path, K)
    tr = Trainer(cfg)
    m = tr.evaluate()
    assert m["batches"] == 2 and m["cases"] == 10 == len(tr.x_test)
    S = 32 * 32
    # the old keys: the two full batches through eval_sums, as before
    old = np.zeros(4)
    for b in range(2):
        x, y = torch.from_numpy(tr.x_test[4 * b:4 * b + 4]), torch.from_numpy(tr.y_test[4 * b:4 * b + 4])
        mb = metrics_from_sums(tr.backend.eval_sums(x, y), y.numel(), cfg)
        old += [mb["loss"], mb["dice"], mb["sensitivity"], mb["specificity"]]
    for k, v in zip(("loss", "dice", "sensitivity", "specificity"), old / 2):
        assert m[k] == v
    # the new keys: the oracle over all 10 cases
    stats = seg_metrics.case_stats_torch(tr.backend.predict(torch.from_numpy(tr.x_test)),
                                         torch.from_numpy(tr.y_test), cfg.eval_threshold)
    want = seg_metrics.metrics_from_case_stats(stats, S)
    pc = m["per_class"]
    assert set(pc) == {"dice", "case_dice", "sensitivity", "specificity"} and all(len(v) == K for v in pc.values())
    for key in ("case_dice", "sensitivity", "specificity"):
        assert np.allclose(pc[key], want[key], rtol=0, atol=1e-12, equal_nan=True), key
    assert m["case_dice"] == pytest.approx(want["case_dice_mean"], abs=1e-12)
    if K == 1:
        # the pooled soft Dice of a single class is the existing `dice` (fp32 sums of B S terms there)
        B = cfg.batch_size
        assert abs(pc["dice"][0] - m["dice"]) <= B * S * 2.0 ** -24 * m["dice"]
    # the report: the existing block unchanged, the new lines after it, JSONL with the new keys
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tr.log.test(3, m, 1, 1, final=True)
    tr.log.close()
    lines = out.getvalue().split("\n")
    assert lines[:6] == ["", "Epoch 1 of 1: TEST DATASET", "loss = {:.4f}".format(m["loss"]),
                         "Dice = {:.4f}".format(m["dice"]), "Sensitivity = {:.4f}".format(m["sensitivity"]),
                         "Specificity = {:.4f}".format(m["specificity"])]
    assert [l.split(":")[0] for l in lines[6:6 + K]] == ["class %d" % k for k in range(K)]
    assert lines[6 + K].startswith("Case Dice = ") and lines[6 + K].endswith("(10 cases)")
    rec = json.loads(open(cfg.log_jsonl).read().strip().split("\n")[-1])
    assert rec["kind"] == "test_final" and rec["cases"] == 10 and len(rec["per_class"]["case_dice"]) == K
    assert {"loss", "dice", "sensitivity", "specificity", "batches", "case_dice"} <= set(rec)


def test_cpu_trainer_test_set_smaller_than_the_batch(tmp_path):
    """Fewer test cases than the per-rank batch: no full batch, every case still scored."""
    from unet_distributed_amd.runtime.trainer import Trainer
    tr = Trainer(_trainer_cfg(tmp_path, 2, batch_size=16, synthetic_train=16))
    m = tr.evaluate()
    assert m["batches"] == 0 and m["cases"] == 10 and m["dice"] == 0.0
    assert all(0.0 <= v <= 1.0 for v in m["per_class"]["case_dice"])


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
    m["len_test"] = len(tr.x_test)
    with open(os.path.join(out, "r%d.json" % rank), "w") as f:
        json.dump(seg_metrics.jsonable(m), f)
    D.destroy()


def test_two_ranks_return_the_same_report(tmp_path):
    mp.spawn(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (json.load(open(tmp_path / ("r%d.json" % r))) for r in range(2))
    assert a == b
    assert a["cases"] == a["len_test"] == 10 and a["batches"] == 2


# ------------------------------------------------------------------ flag and post-hoc check
def test_eval_threshold_flag_bounds():
    from unet_distributed_amd.config import Config, parse_args, validate
    assert Config().eval_threshold == 0.5
    assert parse_args(["--eval_threshold", "0.3"]).eval_threshold == 0.3
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(SystemExit):
            validate(Config(eval_threshold=bad))
    validate(Config(eval_threshold=0.999))


def test_sanity_check_per_class_lines(tmp_path):
    from unet_distributed_amd import sanity_check
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.ops.losses import sanity_dice
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
            avg = sanity_check.main(argv + extra)
        return avg, out.getvalue().split("\n")

    # the text as it is without the flag (reference iteration: batches 0..3 and 4..7 of 10)
    model = load_saved_model(d, device="cpu", batch=4, backend="torch")
    x, y = synthetic_brats(10, 32, 4, 2, seed=1, out_channels=3)
    want_avg = np.mean([sanity_dice(y[s:s + 4].astype(np.float32), model.predict(x[s:s + 4])) for s in (0, 4)])
    avg, plain = run([])
    assert avg == want_avg
    assert plain[:5] == ["Loading trained model from directory {}".format(d), "-" * 38,
                         "Loading and preprocessing test data...", "-" * 38,
                         "Average Dice for Test Set = {}".format(want_avg)]
    assert plain[5].startswith("(2 batches, torch backend, ") and plain[6:] == [""]
    avg2, per = run(["--per_class"])
    assert avg2 == avg and per[:5] == plain[:5]
    stats = model.stats(x[:8], y[:8])
    assert stats.shape == (8, 3, 6)
    want = seg_metrics.metrics_from_case_stats(stats, 32 * 32)
    for k in range(3):
        assert per[5 + k] == "class {}: case Dice = {}, sensitivity = {}, specificity = {}".format(
            k, seg_metrics.fmt(want["case_dice"][k]), seg_metrics.fmt(want["sensitivity"][k]),
            seg_metrics.fmt(want["specificity"][k]))
    assert per[8] == "Case Dice = {} (8 cases)".format(seg_metrics.fmt(want["case_dice_mean"]))
    assert per[9].startswith("(2 batches, torch backend, ")

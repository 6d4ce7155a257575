"""Test-time augmentation off the GPU: the code sets and their order, the flag's validation,
the torch oracle `tta_mean_torch` against a hand-written numpy composition, the ATen
backend's TTA evaluation, the static validation of the executors' `tta_plan`, the plan-time
refusals of the generic ops and the LDS bank model of the tta_acc tile (csrc/kernels/tta.h)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

FW, FH, T, FD = 1, 2, 4, 8


# ------------------------------------------------------------------ code sets and the flag
def test_tta_codes_sets_and_order():
    from unet_distributed_amd.data.augment import ROT90_CODES, tta_codes
    assert tta_codes("", 2) == () and tta_codes("", 3) == ()
    assert tta_codes("flip", 2) == (FW, FH, FW | FH, 0)
    assert tta_codes("flip", 3) == (1, 2, 3, 8, 9, 10, 11, 0)
    assert tta_codes("rot90", 2) == tta_codes("rot90", 3) == (3, 5, 6, 0)
    assert set(tta_codes("rot90", 2)) == set(ROT90_CODES)
    assert tta_codes("flip,rot90", 2) == tuple(range(1, 8)) + (0,)
    assert tta_codes("rot90, flip", 3) == tuple(range(1, 16)) + (0,)
    assert tta_codes(("flip",), 2) == tta_codes("flip", 2)
    for spec in ("flip", "rot90", "flip,rot90"):
        for dims in (2, 3):
            c = tta_codes(spec, dims)
            assert c[-1] == 0 and 0 not in c[:-1] and list(c[:-1]) == sorted(c[:-1])
            assert len(c) & (len(c) - 1) == 0 and len(set(c)) == len(c)


def test_eval_tta_flag_is_validated_like_augment():
    from unet_distributed_amd.config import Config, parse_args, parse_tta, validate
    assert Config().eval_tta == "" and parse_tta("") == ()
    assert parse_args(["--eval_tta", "flip,rot90"]).eval_tta == "flip,rot90"
    assert parse_tta(" rot90 , flip ") == ("rot90", "flip")
    for bad in ("intensity", "flip,intensity", "mirror", "flip,flip", "flip,"):
        with pytest.raises(SystemExit):
            validate(Config(eval_tta=bad))
        with pytest.raises(SystemExit):
            parse_args(["--eval_tta", bad])
    validate(Config(eval_tta="flip", augment="flip,rot90,intensity"))


# ------------------------------------------------------------------ the torch oracle
def _np_apply(a, c):
    """augment.py's source map on a numpy batch [n, (D,) H, W, C], written out per pixel."""
    res = np.empty_like(a)
    out = res
    if a.ndim == 4:
        a, out = a[:, None], res[:, None]
    n, D, H, W, _ = a.shape
    for d in range(D):
        for h in range(H):
            for w in range(W):
                p, q = (w, h) if c & T else (h, w)
                out[:, d, h, w] = a[:, D - 1 - d if c & FD else d, H - 1 - p if c & FH else p,
                                    W - 1 - q if c & FW else q]
    return res


def _np_inverse(c):
    return c ^ (FH | FW) if c & T and bool(c & FH) != bool(c & FW) else c


def _position_fn(shape):
    """A predict_fn that is NOT equivariant: the probability depends on where a pixel sits."""
    g = torch.Generator().manual_seed(11)
    wgt = torch.rand(shape[1:-1] + (1,), generator=g)

    def fn(x):
        return torch.sigmoid(x.sum(-1, keepdim=True) * wgt + 0.25 * wgt)
    return fn


@pytest.mark.parametrize("dims", [2, 3])
def test_tta_mean_torch_equals_a_numpy_composition(dims):
    from unet_distributed_amd.data.augment import inverse_code, tta_codes, tta_mean_torch
    shape = (2, 6, 6, 3) if dims == 2 else (2, 3, 4, 4, 2)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(dims))
    fn = _position_fn(shape)
    codes = tta_codes("flip,rot90", dims)
    assert len(codes) == (8 if dims == 2 else 16)
    for c in codes:
        assert inverse_code(c) == _np_inverse(c)
        assert np.array_equal(_np_apply(_np_apply(x.numpy(), c), _np_inverse(c)), x.numpy())
    got = tta_mean_torch(fn, x, codes)
    acc = None
    for c in codes[:-1]:
        u = _np_apply(fn(torch.from_numpy(_np_apply(x.numpy(), c))).numpy(), _np_inverse(c))
        acc = u if acc is None else acc + u
    want = (acc + fn(x).numpy()) * np.float32(1.0 / len(codes))
    assert want.dtype == np.float32
    assert np.array_equal(got.numpy(), want)
    # the transforms do change this predictor's answer
    assert not torch.equal(got, fn(x))
    for bad in ((0,), (1, 2, 0), (0, 1), (1, 0, 2, 0)):
        with pytest.raises(ValueError):
            tta_mean_torch(fn, x, bad)


@pytest.mark.parametrize("spec,dims", [("flip", 2), ("rot90", 2), ("flip,rot90", 2), ("flip,rot90", 3)])
def test_tta_mean_torch_of_a_pointwise_predictor_is_the_plain_prediction(spec, dims):
    """A pointwise predictor is equivariant: its M probabilities of a pixel are one value p.  The
    running sums 3 p, 5 p, ... of a 24-bit p round in fp32, so the predictor's outputs are
    multiples of 2^-12: every k p, k <= 16, and the division by the power of two M are exact."""
    from unet_distributed_amd.data.augment import tta_codes, tta_mean_torch
    shape = (3, 8, 8, 4) if dims == 2 else (2, 3, 8, 8, 4)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5))

    def fn(t):
        return torch.round(torch.sigmoid(t[..., :2] * 1.7 - t[..., 2:]) * 4096.0) * (1.0 / 4096.0)
    assert torch.equal(tta_mean_torch(fn, x, tta_codes(spec, dims)), fn(x))


# ------------------------------------------------------------------ ATen backend
def _torch_backend(**kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import TorchBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(dtype="fp32", backend="torch", device="cpu", **kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device="cpu")
    flat.load_dict(reference.init_params(spec, seed=3))
    x, y = synthetic_brats(cfg.batch_size, cfg.img_size, cfg.in_channels, cfg.dims, seed=5,
                           out_channels=cfg.out_channels)
    return TorchBackend(spec, flat, cfg, "cpu", cfg.batch_size), torch.from_numpy(x), torch.from_numpy(y)


def test_torch_backend_eval_sums_under_tta():
    from unet_distributed_amd.data.augment import tta_mean_torch
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    kw = dict(batch_size=2, img_size=8, in_channels=2, out_channels=2, depth=2, base_filters=8)
    tb, x, y = _torch_backend(eval_tta="flip", **kw)
    plain, _, _ = _torch_backend(**kw)
    assert tb.tta == (1, 2, 3, 0) and plain.tta == ()
    want = tta_mean_torch(plain.predict, x, (1, 2, 3, 0))
    assert not torch.equal(want, plain.predict(x))                # (a conv net is not flip-equivariant)
    sums = tb.eval_sums(x, y)
    t, p = tb._last_eval
    assert torch.equal(p, want) and torch.equal(tb.predict(x), want)
    t64, p64 = y.double(), want.double()
    bce = torch.nn.functional.binary_cross_entropy(want, y.float(), reduction="sum")
    ref = torch.stack([(t64 * p64).sum(), t64.sum(), p64.sum(), bce.double()])
    assert torch.allclose(sums.double(), ref, rtol=1e-5, atol=0)
    assert torch.equal(sums[3], bce)
    assert torch.equal(tb.last_eval_stats(0.5), case_stats_torch(want, y.float(), 0.5))
    assert torch.equal(tb.eval_stats(x, y, 0.5), case_stats_torch(want, y.float(), 0.5))
    assert torch.equal(tb.eval_surface(x, y, 0.5), case_surface_torch(want, y.float(), 0.5))
    # flag off: the plain forward, BCE from the logits
    assert torch.equal(plain.eval_sums(x, y)[:3].double(),
                       torch.stack([(y.float() * plain.predict(x)).sum(), y.float().sum(),
                                    plain.predict(x).sum()]).double())


def test_predictor_and_config_shim_carry_the_flag():
    from unet_distributed_amd.inference import Predictor, _Cfg
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import UNetSpec
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.data.augment import tta_mean_torch
    assert _Cfg(8, "fp32").eval_tta == "" and _Cfg(8, "fp32", eval_tta="flip").eval_tta == "flip"
    spec = UNetSpec(in_channels=2, n_cl_out=1, base=8, depth=2, use_upsampling=True, dims=2, dropout=0.0)
    flat = FlatParams(spec, device="cpu")
    flat.load_dict(reference.init_params(spec, seed=4))
    x = np.random.RandomState(0).randn(3, 8, 8, 2).astype(np.float32)
    plain = Predictor(spec, flat, 8, "cpu", batch=2)
    tta = Predictor(spec, flat, 8, "cpu", batch=2, tta="rot90")
    want = tta_mean_torch(lambda t: torch.from_numpy(plain.predict(t.numpy())), torch.from_numpy(x), (3, 5, 6, 0))
    assert np.array_equal(tta.predict(x), want.numpy())
    with pytest.raises(SystemExit):
        Predictor(spec, flat, 8, "cpu", batch=2, tta="intensity")


def test_cpu_trainer_evaluates_under_tta(tmp_path, capsys):
    """The ATen backend end to end: start-up line, the report from the mean probabilities over
    every case (two full batches and a padded tail), "tta" in the dict and the JSONL record."""
    import json
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.augment import tta_codes, tta_mean_torch
    from unet_distributed_amd.ops import seg_metrics
    from unet_distributed_amd.runtime.trainer import Trainer
    base = dict(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=16, in_channels=2,
                out_channels=2, depth=2, base_filters=8, device="cpu", backend="torch", dtype="fp32", dropout=0.0,
                checkpoint_dir=str(tmp_path), no_checkpoint=True, tensorboard=False, export=False, resume=False,
                progress=False, eval_hd95=True, log_jsonl=os.path.join(str(tmp_path), "m.jsonl"))
    tr = Trainer(Config(eval_tta="flip,rot90", augment="flip", **base))
    out = capsys.readouterr().out
    assert "Evaluation TTA: flip, rot90 (8 passes)" in out and "Training augmentation: flip" in out
    m = tr.evaluate()
    assert m["tta"] == 8 and m["batches"] == 2 and m["cases"] == 10
    codes = tta_codes("flip,rot90", 2)
    x, y = torch.from_numpy(tr.x_test), torch.from_numpy(tr.y_test).float()
    p = torch.cat([tta_mean_torch(tr.backend._predict1, x[s:s + 4], codes) for s in (0, 4, 8)])
    want = seg_metrics.metrics_from_case_stats(seg_metrics.case_stats_torch(p, y, 0.5), 16 * 16)
    for key in ("case_dice", "sensitivity", "specificity"):
        assert np.allclose(m["per_class"][key], want[key], rtol=0, atol=1e-12, equal_nan=True), key
    hd = seg_metrics.hd95_from_surface(seg_metrics.case_surface_torch(p, y, 0.5), (16, 16)).mean(0)
    assert np.allclose(m["per_class"]["hd95"], hd, rtol=0, atol=1e-9)
    tr.log.test(3, m, 1, 1, final=True)
    tr.log.close()
    rec = json.loads(open(tr.cfg.log_jsonl).read().strip().split("\n")[-1])
    assert rec["kind"] == "test_final" and rec["tta"] == 8
    # flag off: no start-up line, no key
    off = Trainer(Config(**base))
    assert "Evaluation TTA" not in capsys.readouterr().out
    assert "tta" not in off.evaluate() and off.backend.tta == ()
    off.log.close()


# ------------------------------------------------------------------ static plan validation
ENGINES = [
    dict(out_channels=1, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=3, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp16"),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp32"),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dims=3),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, norm="batch"),
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
def test_dry_run_engines_expose_tta_to_plan_check(kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.runtime.plan_check import check_engine, check_stats_plan, check_tta_plan
    cfg = Config(**kw)
    off = _dry_engine(cfg)
    e = _dry_engine(cfg, eval_tta=True)
    # off by default: nothing allocated, and the finding says so
    assert off.tta_plan is None and off.tta_acc_buf is None and off.tta_partial is None
    assert check_tta_plan(off) != []
    assert e.tta_plan.names() == ["tta_acc:write", "tta_acc:add", "tta_finish"]
    assert check_tta_plan(e) == []
    # the existing plans are what they are without the flag
    assert e.plan.names() == off.plan.names() and e.eval_plan.names() == off.eval_plan.names()
    assert all("tta" not in n for n in e.plan.names() + e.eval_plan.names())
    assert check_engine(e) == {"train": [], "eval": []} and check_stats_plan(e) == []
    assert e.tta_acc_buf.shape == e.prob.shape and e.tta_acc_buf.dtype == torch.float32
    assert e.tta_partial.numel() == e.C.tta_finish_blocks(e.prob.numel()) * 4
    with pytest.raises(RuntimeError):
        e.evaluate_tta(torch.zeros(1), torch.zeros(1), (1, 0))   # validated, never launched
    # an extent past either buffer is a named finding
    acc, part = e.tta_acc_buf, e.tta_partial
    e.tta_acc_buf = acc[:-4]
    errs = check_tta_plan(e)
    assert errs and "tta_acc" in errs[0] and "past its end" in errs[0]
    e.tta_acc_buf, e.tta_partial = acc, part[:-1]
    errs = check_tta_plan(e)
    assert errs and "tta_finish" in errs[0] and "past its end" in errs[0]
    e.tta_partial = part
    assert check_tta_plan(e) == []


def test_generic_ops_refuse_bad_arguments_at_plan_time():
    from unet_distributed_amd import native
    C = native.require()
    prob, acc = torch.zeros(2 * 8 * 8 * 4), torch.zeros(2 * 8 * 8 * 4)
    tgt, part, sums = torch.zeros(2 * 8 * 8 * 4), torch.zeros(4 * 4), torch.zeros(4)
    ptrs = [int(prob.data_ptr()), int(acc.data_ptr())]
    plan = C.Plan(0)
    ok = [2, 1, 8, 8, 4, 5, 1]
    plan.add_generic("tta_acc", ptrs, ok, [], "ok")
    plan.add_generic("tta_acc", ptrs, [2, 1, 8, 8, 4, 15, 0], [], "fd ignored in 2D")
    n0 = plan.size()
    bad = [[2, 1, 8, 8, 5, 0, 0], [2, 1, 8, 8, 0, 0, 0],       # K outside 1..4
           [2, 1, 8, 8, 4, 16, 0], [2, 1, 8, 8, 4, -1, 0],     # code outside 0..15
           [2, 1, 8, 8, 4, 0, 2], [2, 1, 8, 8, 4, 0, -1],      # mode
           [2, 1, 8, 4, 4, 0, 0],                              # H != W
           [2, 0, 8, 8, 4, 0, 0], [0, 1, 8, 8, 4, 0, 0],       # D, N >= 1
           [1 << 9, 1, 1024, 1024, 4, 0, 0]]                   # N D H W K = 2^31
    for ints in bad:
        with pytest.raises(ValueError):
            plan.add_generic("tta_acc", ptrs, ints, [], "bad")
        with pytest.raises(ValueError):
            C.generic("tta_acc", ptrs, ints, [], 0)             # (immediate style: nothing launched)
    for null in range(2):
        p = list(ptrs)
        p[null] = 0
        with pytest.raises(ValueError):
            plan.add_generic("tta_acc", p, ok, [], "null")
    with pytest.raises(ValueError):
        plan.add_generic("tta_acc", ptrs, ok[:6], [], "no mode")
    fptrs = [int(t.data_ptr()) for t in (prob, acc, tgt, part, sums)]
    for kind, dt in (("tta_finish", 0), ("tta_finish", 1), ("f32_tta_finish", 0)):
        fplan = C.Plan(dt)
        fplan.add_generic(kind, fptrs, [512], [0.25], "ok")
        for total in (0, 510, 1 << 31):
            with pytest.raises(ValueError):
                fplan.add_generic(kind, fptrs, [total], [0.25], "bad")
        for null in range(5):
            p = list(fptrs)
            p[null] = 0
            with pytest.raises(ValueError):
                fplan.add_generic(kind, p, [512], [0.25], "null")
        with pytest.raises(ValueError):
            fplan.add_generic(kind, [fptrs[0] + 4] + fptrs[1:], [508], [0.25], "unaligned")
        assert fplan.size() == 1
    assert plan.size() == n0
    assert C.tta_finish_blocks(4) == 1 and C.tta_finish_blocks(1024 * 1024 * 4) == 1024
    from unet_distributed_amd.runtime.plan_check import tta_finish_blocks
    for total in (4, 1020, 1024, 1028, 4096 * 3, 1 << 22, 1 << 26):
        assert C.tta_finish_blocks(total) == tta_finish_blocks(total)


# ------------------------------------------------------------------ LDS bank model
def test_tta_tile_pitch_is_conflict_free_for_every_class_count():
    import lds_bank_model as m
    for K in (1, 2, 3, 4):
        assert m.check_tta_tile(K) == (1, 1), K
        # the unpadded tile serialises the transposed reads of a 32-lane half: its 32 / K
        # pixels (11 for K = 3) sit a whole number of bank rows apart
        assert m.check_tta_tile(K, pitch=32 * K) == (1, -(-32 // K)), K

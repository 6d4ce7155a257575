"""Per-(sample, class) evaluation statistics on the GPU: the seg_stats kernel
(csrc/kernels/seg_stats.h) against the float64 oracle (ops/seg_metrics.py), the executors'
`case_stats`, and `Trainer.evaluate`'s per-class / per-case report on the native backend.

Bounds: the counts (slots 3..5) are integers below 2^24 and must equal the oracle's exactly;
a sum (slots 0..2) of S non-negative fp32 terms added in any order is within
S * 2^-24 * |sum| of the exact sum (t p is exact for t in {0, 1}) -- derived, not measured.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SHAPES = [(3, 248), (1, 8), (2, 4096), (2, 262144)]
TDT = {"bf16": (torch.bfloat16, "seg_stats", 0), "fp16": (torch.float16, "seg_stats", 1),
       "fp32": (torch.float32, "f32_seg_stats", 0)}
PAD = 64


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _case(N, S, K, thr, seed):
    """prob uniform in [0, 1] with a share exactly at thr, 0 and 1; target random 0 / 1 with one
    (n, k) all zeros and one all ones."""
    g = torch.Generator().manual_seed(seed)
    prob = torch.rand(N, S, K, generator=g, dtype=torch.float32)
    pick = torch.rand(N, S, K, generator=g)
    prob[pick < 0.10] = torch.tensor(thr, dtype=torch.float32)
    prob[(pick >= 0.10) & (pick < 0.15)] = 0.0
    prob[(pick >= 0.15) & (pick < 0.20)] = 1.0
    target = (torch.rand(N, S, K, generator=g) > 0.6).float()
    target[0, :, 0] = 0.0
    target[N - 1, :, K - 1] = 1.0
    return prob, target


def _launch(prob_d, tgt_d, N, S, K, thr, kind, dtype_id):
    """One launch into a slice of a NaN-filled allocation; returns (stats [N][K][6], guard ok)."""
    chunks = C().seg_stats_chunks(N, S, K)
    big = torch.full((N * K * 6 + 2 * PAD,), float("nan"), dtype=torch.float32, device=prob_d.device)
    out = big[PAD:PAD + N * K * 6]
    part = torch.full((N * chunks * 6 * K,), float("nan"), dtype=torch.float32, device=prob_d.device)
    C().generic(kind, [ptr(prob_d), ptr(tgt_d), ptr(out), ptr(part)], [N, S, K], [thr], stream(), dtype=dtype_id)
    torch.cuda.synchronize()
    guard = bool(torch.isnan(big[:PAD]).all() and torch.isnan(big[PAD + N * K * 6:]).all())
    return out.view(N, K, 6).clone(), guard


def _check(got, want, S, tag):
    got, want = got.double().cpu(), want.double().cpu()
    assert torch.isfinite(got).all(), tag
    assert torch.equal(got[..., 3:], want[..., 3:]), (tag, "counts", got[..., 3:], want[..., 3:])
    err = (got[..., :3] - want[..., :3]).abs()
    bound = S * EPS * want[..., :3].abs()
    print("seg_stats", tag, "max err / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert (err <= bound).all(), (tag, err.max().item())


@pytest.mark.parametrize("tname", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_seg_stats_kernel_matches_float64_oracle(cuda_dev, K, tname):
    """S = 248: S K is no multiple of 12, 16 or 64 for K = 1, 2, 4 (a tail in any lane group)
    and sample boundaries fall mid-wave; S = 262144 is split into several chunks per sample
    (the fixed-order finish); p == thr counts as positive."""
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch
    tdt, kind, dtype_id = TDT[tname]
    for N, S in SHAPES:
        for thr in (0.5, 0.3):
            prob, target = _case(N, S, K, thr, seed=100 * K + N + S % 97)
            want = case_stats_torch(prob, target, thr)
            prob_d, tgt_d = prob.to(cuda_dev), target.to(cuda_dev).to(tdt)
            got, guard = _launch(prob_d, tgt_d, N, S, K, thr, kind, dtype_id)
            tag = "K%d %s N%d S%d thr%.1f" % (K, tname, N, S, thr)
            assert guard, tag + ": wrote outside its stats rows"
            _check(got, want, S, tag)
            # (the case does hold probabilities exactly at the threshold: they count as positive)
            assert S < 248 or int((prob == torch.tensor(thr, dtype=torch.float32)).sum()) > 0
            again, _ = _launch(prob_d, tgt_d, N, S, K, thr, kind, dtype_id)
            assert torch.equal(got, again), tag + ": two runs differ"
    assert C().seg_stats_chunks(2, 262144, K) > 1 and C().seg_stats_chunks(3, 248, K) == 1


# ------------------------------------------------------------------ executors
def _engine(cuda_dev, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(**kw)
    spec = spec_from_config(cfg)
    B = cfg.batch_size
    x, y = synthetic_brats(B, cfg.img_size, cfg.in_channels, cfg.dims, seed=5, out_channels=cfg.out_channels)
    flat = FlatParams(spec, device=cuda_dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    nb = NativeBackend(spec, flat, cfg, cuda_dev, B)
    nb.engine.repack()
    return nb, torch.from_numpy(x).to(cuda_dev), torch.from_numpy(y).to(cuda_dev)


ENGINE_CASES = [
    dict(out_channels=3, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp16", norm="group"),
    dict(out_channels=2, batch_size=2, img_size=16, in_channels=4, dims=3),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp32"),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=lambda kw: "K%d-%s-%dd" % (kw["out_channels"], kw.get("dtype", "bf16"),
                                                                          kw.get("dims", 2)))
def test_executor_case_stats_match_oracle_and_sums(cuda_dev, kw):
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch
    nb, x, y = _engine(cuda_dev, **kw)
    e = nb.engine
    K, B = kw["out_channels"], kw["batch_size"]
    S = e.npix(1) // B
    e.load_batch(x, y)
    e.evaluate_batch()
    for thr in (0.5, 0.3):
        got = e.case_stats(thr)
        torch.cuda.synchronize()
        assert got.shape == (B, K, 6) and got.data_ptr() == e.case_stats_buf.data_ptr()     # (no allocation per call)
        want = case_stats_torch(e.probs().cpu(), e.target.view(B, S, K).float().cpu(), thr)
        _check(got, want, S, "engine %s thr%.1f" % (kw, thr))
    tot = got.double().sum(dim=(0, 1))[:3].cpu()
    sums = e.sums[:3].double().cpu()
    assert ((tot - sums).abs() <= B * S * K * EPS * sums.abs()).all(), (tot, sums)
    assert "case_stats" not in e.plan.names() and "case_stats" not in e.eval_plan.names()


def test_native_eval_stats_pads_a_short_batch(cuda_dev):
    """n < B samples: zero padding to the per-rank batch leaves the real samples' rows as they
    are in a full batch (evaluation normalises per sample or with moving statistics)."""
    nb, x, y = _engine(cuda_dev, out_channels=3, batch_size=4, img_size=32, in_channels=4)
    full = nb.eval_stats(x, y, 0.5).cpu()
    short = nb.eval_stats(x[:3], y[:3], 0.5).cpu()
    assert short.shape == (3, 3, 6) and torch.equal(short, full[:3])
    with pytest.raises(ValueError):
        nb.eval_stats(torch.cat([x, x]), torch.cat([y, y]), 0.5)
    with pytest.raises(ValueError):
        nb.eval_sums(x[:3], y[:3])           # (eval_sums keeps its contract)


def test_predictor_stats_any_length(cuda_dev, tmp_path):
    """Predictor.stats on the native backend: 6 samples at batch 4 (a padded last chunk)."""
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    model = load_saved_model(export_model(cfg, spec, flat), device=cuda_dev, batch=4)
    assert model.name == "native"
    x, y = synthetic_brats(6, 32, 4, seed=2, out_channels=3)
    got = model.stats(x, y, 0.5)
    assert got.shape == (6, 3, 6) and got.dtype == np.float64
    want = case_stats_torch(torch.from_numpy(model.predict(x)), torch.from_numpy(y), 0.5)
    _check(torch.from_numpy(got), want, 32 * 32, "predictor")


# ------------------------------------------------------------------ trainer
def test_trainer_evaluate_reports_per_class_and_per_case(cuda_dev, tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, metrics_from_case_stats
    from unet_distributed_amd.runtime.trainer import Trainer, metrics_from_sums
    cfg = Config(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                 out_channels=3, device="cuda", backend="native", checkpoint_dir=str(tmp_path), no_checkpoint=True,
                 tensorboard=False, export=False, resume=False, progress=False)
    tr = Trainer(cfg)
    assert tr.backend.name == "native" and len(tr.x_test) == 10
    m = tr.evaluate()
    assert m["batches"] == 2 and m["cases"] == 10
    # the five old keys: again through eval_sums
    old = np.zeros(4)
    for b in range(2):
        x = torch.from_numpy(np.ascontiguousarray(tr.x_test[4 * b:4 * b + 4])).to(cuda_dev)
        y = torch.from_numpy(np.ascontiguousarray(tr.y_test[4 * b:4 * b + 4])).to(cuda_dev)
        mb = metrics_from_sums(tr.backend.eval_sums(x, y), y.numel(), cfg)
        old += [mb["loss"], mb["dice"], mb["sensitivity"], mb["specificity"]]
    for k, v in zip(("loss", "dice", "sensitivity", "specificity"), old / 2):
        assert m[k] == v, (k, m[k], v)
    # the new keys: the oracle over backend.predict of all 10 samples (padded last chunk)
    S, K = 32 * 32, 3
    probs = []
    for s in (0, 4, 8):
        xb = torch.from_numpy(np.ascontiguousarray(tr.x_test[s:s + 4])).to(cuda_dev)
        n = xb.shape[0]
        if n < 4:
            xb = torch.cat([xb, xb.new_zeros((4 - n,) + tuple(xb.shape[1:]))])
        probs.append(tr.backend.predict(xb)[:n].cpu())
    stats = case_stats_torch(torch.cat(probs), torch.from_numpy(tr.y_test).float(), 0.5)
    want = metrics_from_case_stats(stats, S)
    for key in ("case_dice", "sensitivity", "specificity"):
        assert np.allclose(m["per_class"][key], want[key], rtol=0, atol=1e-12, equal_nan=True), (key, m, want)
    assert abs(m["case_dice"] - want["case_dice_mean"]) < 1e-12
    per_batch = [metrics_from_case_stats(stats[4 * b:4 * b + 4], S)["dice"] for b in range(2)]
    # numerator and denominator of (2I + 1) / (St + Sp + 1) are each within S 2^-24 relative
    # (sums of per-sample sums that are): the quotient within 2 S 2^-24 plus second-order terms
    tol = 3 * S * EPS
    assert np.allclose(m["per_class"]["dice"], np.mean(per_batch, axis=0), rtol=tol, atol=0), (m, per_batch)

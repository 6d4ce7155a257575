"""Test-time augmentation on the GPU (csrc/kernels/tta.h): tta_acc against `apply_torch`,
tta_finish against torch and a float64 oracle, the executors' `evaluate_tta` bit for bit
against a manual loop through the same executor, and the public paths on the native backend
(`Predictor(tta=)`, `Trainer.evaluate` with --eval_tta).

Exactness: flips and quarter turns are permutations, M is a power of two and the order of the
sum is fixed, so the probabilities are held to torch by `torch.equal` and the thresholded
integers derived from them too.  Bound of the four sums: n non-negative fp32 terms added in any
order are within n 2^-24 of the exact sum, relative; a BCE term carries a few more half-ulps
from the precise logf / log1pf: (n + 8) 2^-24 |sum| -- derived, not measured.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PAD = 64
TDT = {"bf16": (torch.bfloat16, "tta_finish", 0), "fp16": (torch.float16, "tta_finish", 1),
       "fp32": (torch.float32, "f32_tta_finish", 0)}


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ tta_acc
def _acc_launch(prob, acc0, shape5, code, mode, off=0):
    """One launch into a slice of a NaN-guarded allocation holding `acc0` (NaN: write mode);
    returns (acc, guard ok).  `off`: floats by which acc is moved off its 16-byte alignment."""
    n = prob.numel()
    big = torch.full((n + 2 * PAD + off,), float("nan"), dtype=torch.float32, device=prob.device)
    big, acc = big[off:], big[PAD + off:PAD + off + n]
    if acc0 is not None:
        acc.copy_(acc0.reshape(-1))
    C().generic("tta_acc", [ptr(prob), ptr(acc)], list(shape5) + [code, mode], [], stream())
    torch.cuda.synchronize()
    guard = bool(torch.isnan(big[:PAD]).all() and torch.isnan(big[PAD + n:]).all())
    return acc.clone().view(prob.shape), guard


def _acc_case(cuda_dev, K, N, D, H, codes, off=0):
    from unet_distributed_amd.data.augment import apply_torch
    g = torch.Generator().manual_seed(1000 * K + 10 * H + D)
    shape = (N, H, H, K) if D == 1 else (N, D, H, H, K)
    prob = torch.rand(shape, generator=g).to(cuda_dev)
    if off:                                 # (prob too sits `off` floats past a 16-byte boundary)
        prob = torch.cat([prob.new_zeros(off), prob.reshape(-1)])[off:].view(shape)
        assert prob.data_ptr() % 16 == 4 * off
    acc0 = torch.randn(shape, generator=g).to(cuda_dev)
    shape5 = (N, D, H, H, K)
    for c in codes:
        tag = "K%d N%d D%d H%d code %d" % (K, N, D, H, c)
        want = apply_torch(prob, prob, [c] * N)[0]
        got, guard = _acc_launch(prob, None, shape5, c, 0, off)
        assert guard, tag + ": wrote outside acc"
        assert not torch.isnan(got).any(), tag + ": write mode left (or read) a NaN"
        assert torch.equal(got, want), tag + ": write"
        again, _ = _acc_launch(prob, None, shape5, c, 0, off)
        assert torch.equal(got, again), tag + ": two runs differ"
        got, guard = _acc_launch(prob, acc0, shape5, c, 1, off)
        assert guard, tag + ": wrote outside acc (add)"
        assert torch.equal(got, acc0 + want), tag + ": add"
    return prob


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_tta_acc_matches_apply_torch_2d(cuda_dev, K):
    """H = W = 16: the tile and the strip are larger than the image; 48: partial tiles, partial
    strip rows and 3 strips of 16 rows; 128: full-width strips (one contiguous run) and 4 x 4 tiles."""
    for H in (16, 48, 128):
        prob = _acc_case(cuda_dev, K, 3, 1, H, range(8))
    # bits outside the dims are ignored, as the gather ignores them: FD in 2D
    from unet_distributed_amd.data.augment import apply_torch
    got, _ = _acc_launch(prob, None, (3, 1, 128, 128, K), 8 | 5, 0)
    assert torch.equal(got, apply_torch(prob, prob, [5] * 3)[0])


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_tta_acc_odd_rows_and_unaligned_buffers(cuda_dev, K):
    """The codes without the swap move 16-byte vectors when a row is a whole number of them
    and prob / acc are 16-byte aligned (K = 1, 2, 4), flat floats otherwise.  H = W = 18: rows of
    18 K floats -- no whole vectors at K = 1, whole 2-pixel vectors at K = 2 with a partial strip
    column; buffers one float off the alignment take the flat path at every K."""
    _acc_case(cuda_dev, K, 2, 1, 18, range(8))
    _acc_case(cuda_dev, K, 2, 3, 48, range(16), off=1)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_tta_acc_matches_apply_torch_3d(cuda_dev, K):
    _acc_case(cuda_dev, K, 2, 5, 16, range(16))


def test_tta_acc_inverse_code_brings_the_gathered_batch_back(cuda_dev):
    """acc of inverse_code(c) applied to apply_torch(p, c) is p: the caller's contract."""
    from unet_distributed_amd.data.augment import apply_torch, inverse_code
    p = torch.rand(2, 3, 48, 48, 3, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    for c in range(16):
        moved = apply_torch(p, p, [c] * 2)[0]
        got, guard = _acc_launch(moved, None, (2, 3, 48, 48, 3), inverse_code(c), 0)
        assert guard and torch.equal(got, p), c


# ------------------------------------------------------------------ tta_finish
def _bce64(p, t):
    lp = torch.log(p).clamp_min(-100.0)
    lq = torch.log1p(-p).clamp_min(-100.0)
    return -(t * lp + (1.0 - t) * lq).sum()


def _sums64(p, t):
    p, t = p.double().reshape(-1), t.double().reshape(-1)
    return torch.stack([(t * p).sum(), t.sum(), p.sum(), _bce64(p, t)])


def _check_sums(got, want, n, tag):
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    bound = (n + 8) * EPS * want.abs()
    print("tta sums", tag, "err / bound", [float(v) for v in err / bound.clamp_min(1e-300)])
    assert torch.isfinite(got).all() and (err <= bound).all(), (tag, got, want)


@pytest.mark.parametrize("tname", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("M", [4, 8, 16])
def test_tta_finish_mean_and_sums(cuda_dev, M, tname):
    """total = 4 * 12345: 49 blocks, the last one partly idle; 4 * (1024 * 256 + 77): more vectors
    than lanes in the 1024-block grid (the grid-stride pass).  The means include exact 0 and 1."""
    tdt, kind, dtype_id = TDT[tname]
    for total in (4 * 12345, 4 * (1024 * 256 + 77)):
        g = torch.Generator().manual_seed(M + total % 89)
        prob = torch.rand(total, generator=g)
        acc = torch.rand(total, generator=g) * (M - 1)
        pick = torch.rand(total, generator=g)
        prob[pick < 0.05], acc[pick < 0.05] = 0.0, 0.0
        prob[pick > 0.95], acc[pick > 0.95] = 1.0, float(M - 1)
        tgt = (torch.rand(total, generator=g) > 0.6).float()
        prob_d, acc_d, tgt_d = prob.to(cuda_dev), acc.to(cuda_dev), tgt.to(cuda_dev).to(tdt)
        want = (acc_d + prob_d) * (1.0 / M)
        assert float(want.min()) == 0.0 and float(want.max()) == 1.0
        nb = C().tta_finish_blocks(total)
        runs = []
        for _ in range(2):
            p = prob_d.clone()
            part = torch.full((nb * 4,), float("nan"), dtype=torch.float32, device=cuda_dev)
            big = torch.full((4 + 2 * PAD,), float("nan"), dtype=torch.float32, device=cuda_dev)
            sums = big[PAD:PAD + 4]
            C().generic(kind, [ptr(p), ptr(acc_d), ptr(tgt_d), ptr(part), ptr(sums)], [total], [1.0 / M], stream(),
                        dtype=dtype_id)
            torch.cuda.synchronize()
            assert torch.isnan(big[:PAD]).all() and torch.isnan(big[PAD + 4:]).all()
            assert not torch.isnan(part).any()
            runs.append((p, sums.clone()))
        tag = "M%d %s total %d" % (M, tname, total)
        assert torch.equal(runs[0][0], want), tag
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), tag + ": two runs differ"
        _check_sums(runs[0][1], _sums64(want.cpu(), tgt), total, tag)


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


def _manual_tta(e, x, y, codes):
    """The oracle: every pass through the same executor's plain load and evaluation plan, the
    un-augmentation and the mean in torch (`tta_mean_torch`'s arithmetic)."""
    from unet_distributed_amd.data.augment import apply_torch, tta_mean_torch

    def predict(xa):
        # (the transformed target rides along as in evaluate_tta; the probabilities do not read it)
        c = calls.pop(0)
        ya = apply_torch(y, y, [c] * y.shape[0])[0]
        e.load_batch(xa.contiguous(), ya.contiguous())
        e.evaluate_batch()
        return e.probs().clone()
    calls = list(codes)
    out = tta_mean_torch(predict, x, codes)
    assert not calls
    return out


ENGINE_CASES = [
    dict(out_channels=1, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=3, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=1, batch_size=4, img_size=32, in_channels=4, dtype="fp16"),
    dict(out_channels=1, batch_size=4, img_size=32, in_channels=4, dtype="fp32"),
    dict(out_channels=1, batch_size=4, img_size=32, in_channels=4, norm="batch"),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dims=3),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=lambda kw: "K%d-%s-%s-%dd" % (
    kw["out_channels"], kw.get("dtype", "bf16"), kw.get("norm", "none"), kw.get("dims", 2)))
def test_evaluate_tta_is_bit_exact_against_a_manual_loop(cuda_dev, kw):
    from unet_distributed_amd.data.augment import tta_codes
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    nb, x, y = _engine(cuda_dev, **kw)
    e = nb.engine
    dims, B, K = kw.get("dims", 2), kw["batch_size"], kw["out_channels"]
    assert e.tta_plan is None and e.tta_acc_buf is None            # off: nothing allocated
    codes = tta_codes("flip,rot90", dims)
    assert len(codes) == (16 if dims == 3 else 8)
    want = _manual_tta(e, x, y, codes)
    e.evaluate_tta(x, y, codes)
    torch.cuda.synchronize()
    got = e.probs().clone()
    assert torch.equal(got, want)
    e.load_batch(x, y)
    plain = e.target.clone()
    e.evaluate_batch()
    assert not torch.equal(e.probs(), want)                        # (the network is not equivariant)
    e.evaluate_tta(x, y, codes)
    assert torch.equal(e.probs(), got), "two runs differ"
    assert torch.equal(e.target, plain), "the identity pass must leave the stored target behind"
    S = e.npix(1) // B
    _check_sums(e.sums, _sums64(want.cpu(), y.cpu()), B * S * K, "engine %s" % kw)
    stats = e.case_stats(0.5).clone()
    ref = case_stats_torch(want.cpu(), y.float().cpu(), 0.5)
    assert torch.equal(stats[..., 3:].double().cpu(), ref[..., 3:].double())
    assert torch.equal(e.case_surface(0.5).long().cpu(), case_surface_torch(want.cpu(), y.float().cpu(), 0.5).long())
    # flip alone: a second code set on the same executor (its own code rows)
    flip = tta_codes("flip", dims)
    e.evaluate_tta(x, y, flip)
    got = e.probs().clone()                 # (a view of the executor's buffer, which the oracle's passes reuse)
    assert torch.equal(got, _manual_tta(e, x, y, flip))
    assert set(e._tta_rows) == {codes, flip}
    for bad in ((0,), (1, 2, 0), (0, 1), (1, 1, 2, 0)):
        with pytest.raises(ValueError):
            e.evaluate_tta(x, y, bad)
    with pytest.raises(ValueError):
        e.evaluate_tta(x[:1], y[:1], flip)


def test_ops_of_eval_sums_with_the_flag_off_are_the_parents(cuda_dev, monkeypatch):
    """eval_tta = "": one eval_sums issues the plain gather and the evaluation plan, no tta_*
    op, and allocates no TTA buffer; with the flag the gathers augment and the tta ops follow."""
    issued = []
    nb, x, y = _engine(cuda_dev, out_channels=1, batch_size=4, img_size=32, in_channels=4)
    on, _, _ = _engine(cuda_dev, out_channels=1, batch_size=4, img_size=32, in_channels=4, eval_tta="flip")
    real = nb.engine.C.generic

    class Spy:
        def __init__(self, mod):
            self._mod = mod

        def generic(self, kind, *a, **k):
            issued.append(kind)
            return real(kind, *a, **k)

        def __getattr__(self, name):
            return getattr(self._mod, name)
    for b in (nb, on):
        monkeypatch.setattr(b.engine, "C", Spy(b.engine.C))
        runs = []

        def evaluate_batch(stream=None, _real=b.engine.evaluate_batch):
            runs.append(stream)
            return _real(stream)
        monkeypatch.setattr(b.engine, "evaluate_batch", evaluate_batch)
        del issued[:]
        b.eval_sums(x, y)
        torch.cuda.synchronize()
        if b is nb:
            assert issued == ["gather_batch"] and len(runs) == 1
            assert b.engine.tta_plan is None and b.engine.tta_acc_buf is None and b.engine.tta_partial is None
        else:
            assert issued == ["gather_batch_aug", "tta_acc"] * 3 + ["gather_batch_aug", "tta_finish"]
            assert len(runs) == 4 and b.engine.tta_acc_buf is not None
    assert nb.tta == () and on.tta == (1, 2, 3, 0)


# ------------------------------------------------------------------ public paths
def test_predictor_tta_pads_a_short_chunk(cuda_dev, tmp_path):
    """Predictor(tta="flip").predict on 5 samples at batch 4: the padded last chunk too."""
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.augment import tta_codes
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    export = export_model(cfg, spec, flat)
    model = load_saved_model(export, device=cuda_dev, batch=4, tta="flip")
    plain = load_saved_model(export, device=cuda_dev, batch=4)
    assert model.name == "native" and model.backend.tta == (1, 2, 3, 0) and plain.backend.tta == ()
    x, y = synthetic_brats(5, 32, 4, seed=2, out_channels=3)
    e = plain.backend.engine
    want = []
    for s in (0, 4):
        xb = torch.from_numpy(x[s:s + 4]).to(cuda_dev)
        n = xb.shape[0]
        if n < 4:
            xb = torch.cat([xb, xb.new_zeros((4 - n,) + tuple(xb.shape[1:]))])
        yb = torch.zeros(xb.shape[:-1] + (3,), device=cuda_dev)
        want.append(_manual_tta(e, xb, yb, tta_codes("flip", 2))[:n].cpu())
    want = torch.cat(want)
    got = model.predict(x)
    assert got.shape == (5, 32, 32, 3) and np.array_equal(got, want.numpy())
    assert not np.array_equal(got, plain.predict(x))
    ref = case_stats_torch(want, torch.from_numpy(y), 0.5)
    assert np.array_equal(model.stats(x, y, 0.5)[..., 3:], ref[..., 3:].double().numpy())
    assert np.array_equal(model.surface(x, y, 0.5), case_surface_torch(want, torch.from_numpy(y), 0.5).long().numpy())


def test_trainer_evaluate_under_tta(cuda_dev, tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.augment import tta_codes
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, metrics_from_case_stats
    from unet_distributed_amd.runtime.trainer import Trainer
    cfg = Config(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                 out_channels=3, device="cuda", backend="native", checkpoint_dir=str(tmp_path), no_checkpoint=True,
                 tensorboard=False, export=False, resume=False, progress=False, eval_tta="flip,rot90")
    tr = Trainer(cfg)
    assert tr.backend.name == "native" and len(tr.x_test) == 10 and tr.backend.engine.tta_plan is not None
    m = tr.evaluate()
    assert m["tta"] == 8 and m["batches"] == 2 and m["cases"] == 10
    e = tr.backend.engine
    codes = tta_codes("flip,rot90", 2)
    probs = []
    for s in (0, 4, 8):
        xb = torch.from_numpy(np.ascontiguousarray(tr.x_test[s:s + 4])).to(cuda_dev)
        yb = torch.from_numpy(np.ascontiguousarray(tr.y_test[s:s + 4])).to(cuda_dev)
        n = xb.shape[0]
        if n < 4:
            xb = torch.cat([xb, xb.new_zeros((4 - n,) + tuple(xb.shape[1:]))])
            yb = torch.cat([yb, yb.new_zeros((4 - n,) + tuple(yb.shape[1:]))])
        probs.append(_manual_tta(e, xb, yb, codes)[:n].cpu())
    stats = case_stats_torch(torch.cat(probs), torch.from_numpy(tr.y_test).float(), 0.5)
    want = metrics_from_case_stats(stats, 32 * 32)
    for key in ("case_dice", "sensitivity", "specificity"):
        assert np.allclose(m["per_class"][key], want[key], rtol=0, atol=1e-12, equal_nan=True), (key, m, want)
    assert abs(m["case_dice"] - want["case_dice_mean"]) < 1e-12

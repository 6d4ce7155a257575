"""Surface distances for HD95 on the GPU: the surf_dist kernels (csrc/kernels/surf_dist.h)
against the all-pairs oracle (ops/seg_metrics.py) by torch.equal -- the kernel output is four
integers per (sample, class), so there is no tolerance -- the sample grouping, the executors'
`case_surface`, `NativeBackend.eval_surface`, `Trainer.evaluate` with --eval_hd95 and
`Predictor.surface`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# [N, D, H, W]: smallest (a sample boundary mid-wave) | non-square | the model's slice | a
# squared distance past 16 bits on a 512-wide row | smallest 3D | 3D | a long D axis | the
# largest LDS tile of a line pass (64 lines of 120: 62 KiB)
SHAPES = [(3, 1, 8, 8), (2, 1, 16, 24), (2, 1, 128, 128), (1, 1, 8, 512), (2, 4, 8, 8), (1, 32, 32, 32),
          (1, 128, 16, 8), (1, 1, 72, 120)]
TDT = {"bf16": (torch.bfloat16, "surf_dist", 0), "fp16": (torch.float16, "surf_dist", 1),
       "fp32": (torch.float32, "f32_surf_dist", 0)}
PAD = 64
GUARD = 0x5A5A5A5A
NCASE = 9


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _thr(K):
    return 0.3 if K % 2 == 0 else 0.5


def _blob(rng, grid):
    """Sparse random seeds dilated by one or two face-neighbour steps (small surfaces keep the
    all-pairs oracle small)."""
    m = np.zeros(grid, dtype=bool)
    for _ in range(max(2, int(np.prod(grid)) // 400)):
        m[tuple(rng.randint(0, v) for v in grid)] = True
    for _ in range(rng.randint(1, 3)):
        g = m.copy()
        for ax in range(3):
            if grid[ax] > 1:
                lo, hi = [slice(None)] * 3, [slice(None)] * 3
                lo[ax], hi[ax] = slice(0, -1), slice(1, None)
                g[tuple(hi)] |= m[tuple(lo)]
                g[tuple(lo)] |= m[tuple(hi)]
        m = g
    return m


def _slot(rng, grid, case, thr):
    """(prob fp32, target 0/1) of one (sample, class) on grid (D, H, W); `case` picks a forced
    situation, 0 the plain random one."""
    hi_p, lo_p = np.float32(0.9), np.float32(0.1)
    P, T = _blob(rng, grid), _blob(rng, grid)
    if case == 1:
        P[:] = False                                     # empty P
    elif case == 2:
        T[:] = False                                     # empty T
    elif case == 3:
        P[:] = False                                     # both empty
        T[:] = False
    elif case == 4:
        P[:] = True                                      # full foreground: its surface is the border
    elif case == 5:
        P[:] = False                                     # single voxels in opposite corners:
        T[:] = False                                     # the largest distance of the shape
        P[0, 0, 0] = True
        T[-1, -1, -1] = True
    elif case == 6:
        T[:] = False                                     # T = P shifted by 3 voxels along W: many ties
        T[:, :, 3:] = P[:, :, :-3]
    elif case == 7:
        P[:] = False                                     # one voxel each: m = 2
        T[:] = False
        P[tuple(rng.randint(0, v) for v in grid)] = True
        T[tuple(rng.randint(0, v) for v in grid)] = True
    prob = np.where(P, hi_p, lo_p).astype(np.float32)
    if case == 8:                                        # exactly at the threshold inside (surface
        t32 = np.float32(thr)                            # voxels included), the next float below outside
        prob = np.where(P, t32, np.nextafter(t32, np.float32(0))).astype(np.float32)
    return prob, T.astype(np.float32)


_CASES = {}


def _case_id(shape, K, n, k):
    """The situation of slot (n, k): they rotate with the shape and K so that every one is
    reached; the 512-wide row always holds the opposite corners."""
    if shape[3] == 512 and n == 0 and k == 0:
        return 5
    si = SHAPES.index(shape) if shape in SHAPES else len(SHAPES)
    return (n * K + k + 2 * si + K) % NCASE


def _case(shape, K):
    """(prob [N][S][K], target [N][S][K], oracle int64 [N][K][4], thr) of a shape: built and
    scored once, shared by every test and target type (0 / 1 targets are exact in all three)."""
    from unet_distributed_amd.ops.seg_metrics import case_surface_torch
    if (shape, K) not in _CASES:
        N, grid = shape[0], tuple(shape[1:])
        thr = _thr(K)
        rng = np.random.RandomState(1000 * sum(shape) + K)
        prob = np.zeros((N,) + grid + (K,), dtype=np.float32)
        tgt = np.zeros((N,) + grid + (K,), dtype=np.float32)
        for n in range(N):
            for k in range(K):
                prob[n, ..., k], tgt[n, ..., k] = _slot(rng, grid, _case_id(shape, K, n, k), thr)
        prob, tgt = torch.from_numpy(prob), torch.from_numpy(tgt)
        S = int(np.prod(grid))
        _CASES[(shape, K)] = (prob.view(N, S, K), tgt.view(N, S, K), case_surface_torch(prob, tgt, thr), thr)
    return _CASES[(shape, K)]


def _launch(prob_d, tgt_d, shape, K, thr, kind, dtype_id, fill=0xFF):
    """One launch into slices of guard-filled allocations, the scratch pre-filled with `fill`
    bytes; returns (surf int32 [N][K][4], guards intact)."""
    N, D, H, W = shape
    dev = prob_d.device
    big = torch.full((N * K * 4 + 2 * PAD,), GUARD, dtype=torch.int32, device=dev)
    out = big[PAD:PAD + N * K * 4]
    words = C().surf_dist_scratch(N, D, H, W, K) // 4
    sbig = torch.full((words + 2 * PAD,), GUARD, dtype=torch.int32, device=dev)
    scratch = sbig[PAD:PAD + words]
    scratch.view(torch.uint8).fill_(fill)
    C().generic(kind, [ptr(prob_d), ptr(tgt_d), ptr(out), ptr(scratch)], [N, D, H, W, K], [thr], stream(), dtype=dtype_id)
    torch.cuda.synchronize()
    guard = bool((big[:PAD] == GUARD).all() and (big[PAD + N * K * 4:] == GUARD).all() and
                 (sbig[:PAD] == GUARD).all() and (sbig[PAD + words:] == GUARD).all())
    return out.view(N, K, 4).clone(), guard


@pytest.mark.parametrize("tname", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_surf_dist_kernel_equals_the_all_pairs_oracle(cuda_dev, K, tname):
    tdt, kind, dtype_id = TDT[tname]
    for shape in SHAPES:
        prob, tgt, want, thr = _case(shape, K)
        got, guard = _launch(prob.to(cuda_dev), tgt.to(cuda_dev).to(tdt), shape, K, thr, kind, dtype_id)
        tag = "K%d %s %s" % (K, tname, shape)
        assert guard, tag + ": wrote outside its output rows or its scratch"
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu().long(), want), (tag, got.cpu().tolist(), want.tolist())


def test_forced_cases_are_all_reached():
    """The slots of the kernel test do hold each forced situation (checked on the oracle)."""
    seen = set()
    for shape in SHAPES:
        for K in (1, 2, 3, 4):
            want = _case(shape, K)[2]
            for n in range(shape[0]):
                for k in range(K):
                    seen.add(_case_id(shape, K, n, k))
                    mp, mt, lo, hi = want[n, k].tolist()
                    assert (lo == -1) == (mp == 0 or mt == 0) and lo <= hi
    assert seen == set(range(NCASE))
    # the 512-wide row: opposite corners are 7^2 + 511^2 apart, past 16 bits
    hit = [_case((1, 1, 8, 512), K)[2] for K in (1, 2, 3, 4)]
    assert any((w[..., 2] == 7 * 7 + 511 * 511).any() for w in hit)


@pytest.mark.parametrize("shape", [(2, 1, 16, 24), (2, 4, 8, 8)])
def test_two_runs_give_the_same_bits_whatever_the_scratch_held(cuda_dev, shape):
    K = 3
    prob, tgt, want, thr = _case(shape, K)
    prob_d, tgt_d = prob.to(cuda_dev), tgt.to(cuda_dev).to(torch.bfloat16)
    a, ga = _launch(prob_d, tgt_d, shape, K, thr, "surf_dist", 0, fill=0xFF)
    b, gb = _launch(prob_d, tgt_d, shape, K, thr, "surf_dist", 0, fill=0x00)
    assert ga and gb and torch.equal(a, b) and torch.equal(a.cpu().long(), want)


def test_sample_groups_through_a_small_scratch(cuda_dev):
    """Five samples through a scratch sized for two: three launches, the one-group result."""
    from unet_distributed_amd.runtime.executor_base import launch_surf_dist
    shape, K = (5, 1, 16, 24), 2
    N, D, H, W = shape
    prob, tgt, want, thr = _case(shape, K)
    prob_d, tgt_d = prob.to(cuda_dev), tgt.to(cuda_dev).to(torch.bfloat16)
    one, guard = _launch(prob_d, tgt_d, shape, K, thr, "surf_dist", 0)
    assert guard and torch.equal(one.cpu().long(), want)
    two = C().surf_dist_scratch(2, D, H, W, K)
    sbig = torch.full((two // 4 + 2 * PAD,), GUARD, dtype=torch.int32, device=cuda_dev)
    out = torch.full((N, K, 4), GUARD, dtype=torch.int32, device=cuda_dev)
    launches = launch_surf_dist(C(), "surf_dist", [ptr(prob_d), ptr(tgt_d), ptr(out), ptr(sbig[PAD:])], [N, D, H, W, K],
                                thr, two, 2, stream(), 0)
    torch.cuda.synchronize()
    assert launches == 3
    assert torch.equal(out, one)
    assert bool((sbig[:PAD] == GUARD).all() and (sbig[PAD + two // 4:] == GUARD).all())


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
def test_executor_case_surface_matches_the_oracle(cuda_dev, kw):
    from unet_distributed_amd.ops.seg_metrics import case_surface_torch
    nb, x, y = _engine(cuda_dev, **kw)
    e = nb.engine
    K, B = kw["out_channels"], kw["batch_size"]
    assert e.case_surface_buf is None and e.case_surface_scratch is None      # lazily: not before the first use
    e.load_batch(x, y)
    e.evaluate_batch()
    grid = tuple(e.sdims(1))
    for thr in (0.5, 0.3):
        got = e.case_surface(thr)
        torch.cuda.synchronize()
        assert got.shape == (B, K, 4) and got.dtype == torch.int32
        assert got.data_ptr() == e.case_surface_buf.data_ptr()                # (no allocation per call)
        want = case_surface_torch(e.probs().cpu(), e.target.view((B,) + grid + (K,)).float().cpu(), thr)
        assert torch.equal(got.cpu().long(), want), (kw, thr, got.cpu().tolist(), want.tolist())
        st = e.case_stats(thr).cpu()
        torch.cuda.synchronize()
        assert torch.equal(st[..., 3] + st[..., 4] == 0, got.cpu()[..., 0] == 0)      # TP + FP == 0 <=> mp == 0
        assert torch.equal(st[..., 3] + st[..., 5] == 0, got.cpu()[..., 1] == 0)      # TP + FN == 0 <=> mt == 0
    assert e.surface_plan.names() == ["case_surface"] and e.stats_plan.names() == ["case_stats"]
    assert "case_surface" not in e.plan.names() and "case_surface" not in e.eval_plan.names()


def test_native_eval_surface_pads_a_short_batch(cuda_dev):
    nb, x, y = _engine(cuda_dev, out_channels=3, batch_size=4, img_size=32, in_channels=4)
    full = nb.eval_surface(x, y, 0.5).cpu()
    short = nb.eval_surface(x[:3], y[:3], 0.5).cpu()
    assert full.shape == (4, 3, 4) and short.shape == (3, 3, 4) and torch.equal(short, full[:3])
    nb.eval_sums(x, y)
    assert torch.equal(nb.last_eval_surface(0.5).cpu(), full)
    with pytest.raises(ValueError):
        nb.eval_surface(torch.cat([x, x]), torch.cat([y, y]), 0.5)


def test_predictor_surface_any_length(cuda_dev, tmp_path):
    """Predictor.surface on the native backend: 6 samples at batch 4 (a padded last chunk)."""
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.ops.seg_metrics import case_surface_torch
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    model = load_saved_model(export_model(cfg, spec, flat), device=cuda_dev, batch=4)
    assert model.name == "native"
    x, y = synthetic_brats(6, 32, 4, seed=2, out_channels=3)
    got = model.surface(x, y, 0.5)
    assert got.shape == (6, 3, 4) and got.dtype == np.int64
    want = case_surface_torch(torch.from_numpy(model.predict(x)), torch.from_numpy(y).float(), 0.5)
    assert np.array_equal(got, want.numpy())


# ------------------------------------------------------------------ trainer
def test_trainer_evaluate_reports_hd95(cuda_dev, tmp_path):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.ops.seg_metrics import case_surface_torch, hd95_from_surface
    from unet_distributed_amd.runtime.trainer import Trainer
    cfg = Config(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                 out_channels=3, device="cuda", backend="native", checkpoint_dir=str(tmp_path), no_checkpoint=True,
                 tensorboard=False, export=False, resume=False, progress=False, eval_hd95=True)
    tr = Trainer(cfg)
    assert tr.backend.name == "native" and len(tr.x_test) == 10
    assert tr.backend.engine.case_surface_buf is not None                     # planned with the flag
    m = tr.evaluate()
    assert m["batches"] == 2 and m["cases"] == 10
    # the oracle over backend.predict of all 10 samples (two full batches and a padded tail of 2)
    probs = []
    for s in (0, 4, 8):
        xb = torch.from_numpy(np.ascontiguousarray(tr.x_test[s:s + 4])).to(cuda_dev)
        n = xb.shape[0]
        if n < 4:
            xb = torch.cat([xb, xb.new_zeros((4 - n,) + tuple(xb.shape[1:]))])
        probs.append(tr.backend.predict(xb)[:n].cpu())
    surf = case_surface_torch(torch.cat(probs), torch.from_numpy(tr.y_test).float(), 0.5)
    want = hd95_from_surface(surf, (32, 32)).mean(0)
    assert set(m["per_class"]) == {"dice", "case_dice", "sensitivity", "specificity", "hd95"}
    assert np.allclose(m["per_class"]["hd95"], want, rtol=0, atol=1e-9), (m["per_class"]["hd95"], want)
    assert abs(m["hd95"] - want.mean()) <= 1e-9

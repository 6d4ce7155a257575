"""Connected-component filtering on the GPU: the components op (csrc/kernels/components.h)
against its torch definition (ops/components.py) by torch.equal -- the outputs are integers and
floats that are either copied or 0.0, so there is no tolerance anywhere -- the sample grouping,
the executors' `components` with `case_stats` / `case_surface` on the filtered map,
`NativeBackend`, `Trainer.evaluate` with --eval_components and `Predictor`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# The op has no LDS tile: runs are seeded over the 64 lanes of a wave, CC_SEG = 64 consecutive
# voxels of the linear index cut at row starts, and everything else is unions on the global
# label plane.  The seam shape is just past that segment along W with odd H and D, so that
# runs cross a segment seam at a different offset in every row and S is no multiple of 64.
CC_SEG = 64
# [N, D, H, W]: a sample boundary inside a wave | non-square | the model's slice | a row wider
# than any segment | smallest 3D | 3D | long D | dimensions that divide nothing | the seam
SHAPES = [(3, 1, 8, 8), (2, 1, 16, 24), (2, 1, 128, 128), (1, 1, 8, 512), (2, 4, 8, 8), (1, 32, 32, 32),
          (1, 128, 16, 8), (1, 1, 72, 120), (2, 3, 5, CC_SEG + 1)]
# (K, threshold, keep_largest, min_size): K in 1..3, both thresholds, the three policies
COMBOS = [(1, 0.5, True, 0), (2, 0.3, False, 5), (3, 0.5, True, 5), (1, 0.3, True, 4), (2, 0.5, True, 0),
          (3, 0.3, False, 4)]
PAD = 64
GUARD = 0x5A5A5A5A
NCASE = 11
NAMES = ["random blobs", "empty", "full", "single voxel", "checkerboard", "serpentine", "U-shape",
         "diagonal contact", "two equal blobs", "first-to-last blob", "at threshold"]


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _blob(rng, grid):
    """Sparse random seeds dilated by one or two face-neighbour steps (test_gpu_hd95.py::_blob)."""
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


def _mask(rng, grid, case):
    """Foreground of one (sample, class) on grid (D, H, W); `case` picks the situation (NAMES)."""
    D, H, W = grid
    m = np.zeros(grid, dtype=bool)
    if case in (0, 10):
        m = _blob(rng, grid)
    elif case == 2:
        m[:] = True
    elif case == 3:
        m[tuple(rng.randint(0, v) for v in grid)] = True
    elif case == 4:                                      # every foreground voxel its own component
        z, y, x = np.indices(grid)
        m = (z + y + x) % 2 == 0
    elif case == 5:                                      # one component; its label travels every row and plane
        last = (H - 1) // 2 * 2
        for z in range(0, D, 2):
            m[z, 0::2, :] = True
            for i, y in enumerate(range(1, last, 2)):
                m[z, y, W - 1 if i % 2 == 0 else 0] = True
        for z in range(1, D, 2):                         # an odd plane: one voxel joining its neighbours
            if (z // 2) % 2 == 0:
                m[z, last, W - 1] = True
            else:
                m[z, 0, 0] = True
    elif case == 6:                                      # arms that join only in the last row / plane
        if D > 1:
            m[:, 0, 0] = True
            m[:, H - 1, W - 1] = True
            m[D - 1] = True
        else:
            m[0, :, 0] = True
            m[0, :, W - 1] = True
            m[0, H - 1, :] = True
    elif case == 7:                                      # voxels that touch only diagonally
        for i in range(min(H, W)):
            m[(i % D) if D > 1 else 0, i, i] = True
    elif case == 8:                                      # two blobs of 4 voxels: the smaller label wins
        m[0, 1:3, 1:3] = True
        m[D - 1, H - 3:H - 1, W - 3:W - 1] = True
    elif case == 9:                                      # holds voxel 0 and voxel S - 1: neighbours in memory
        m[:, :, 0] = True                                # of the next sample / class must not merge
        m[0, 0, :] = True
        m[D - 1, H - 1, :] = True
    return m


def _slot(rng, grid, case, thr):
    """fp32 probabilities of one (sample, class): random values >= thr inside the mask and random
    values below it outside (they must pass through bit for bit); case 10: exactly thr inside,
    the next float below outside."""
    m = _mask(rng, grid, case)
    t32 = np.float32(thr)
    if case == 10:
        return np.where(m, t32, np.nextafter(t32, np.float32(0))).astype(np.float32)
    hi = np.maximum(rng.uniform(thr, 1.0, grid).astype(np.float32), t32)
    lo = np.minimum(rng.uniform(0.0, thr, grid).astype(np.float32), np.nextafter(t32, np.float32(0)))
    return np.where(m, hi, lo).astype(np.float32)


def _case_id(shape, combo, n, k):
    """The situation of slot (n, k) of a combo: a running count of the shape's slots over the
    combos, so that every shape reaches every situation (12 N slots, NCASE = 11)."""
    ci = COMBOS.index(combo)
    before = sum(c[0] for c in COMBOS[:ci]) * shape[0]
    si = SHAPES.index(shape) if shape in SHAPES else len(SHAPES)
    return (before + n * combo[0] + k + si) % NCASE


_CASES = {}


def _case(shape, combo):
    """(prob [N, (D,) H, W, K] as the oracle takes it, oracle out, oracle info) of a shape and
    combo: built and scored once, shared by every test."""
    from unet_distributed_amd.ops.components import components_torch
    if (shape, combo) not in _CASES:
        K, thr, largest, min_size = combo
        N, grid = shape[0], tuple(shape[1:])
        rng = np.random.RandomState(1000 * sum(shape) + 7 * COMBOS.index(combo) if combo in COMBOS else 1)
        prob = np.zeros((N,) + grid + (K,), dtype=np.float32)
        for n in range(N):
            for k in range(K):
                prob[n, ..., k] = _slot(rng, grid, _case_id(shape, combo, n, k) if combo in COMBOS else (n + k) % NCASE,
                                        thr)
        prob = torch.from_numpy(prob)
        out, info = components_torch(prob, thr, largest, min_size)
        _CASES[(shape, combo)] = (prob, out, info)
    return _CASES[(shape, combo)]


def _launch(prob_d, shape, combo, fill=0xFF, group=None):
    """One op (or, with `group`, the grouped launches) into slices of guard-filled allocations,
    the scratch pre-filled with `fill` bytes; returns (out, info, guards intact, launches)."""
    from unet_distributed_amd.runtime.executor_base import launch_components
    K, thr, largest, min_size = combo
    N, D, H, W = shape
    dev = prob_d.device
    n_out = N * D * H * W * K
    obig = torch.full((n_out + 2 * PAD,), GUARD, dtype=torch.int32, device=dev)
    out = obig[PAD:PAD + n_out].view(torch.float32)
    ibig = torch.full((N * K * 4 + 2 * PAD,), GUARD, dtype=torch.int32, device=dev)
    info = ibig[PAD:PAD + N * K * 4]
    g = group or N
    words = C().components_scratch(g, D, H, W, K) // 4
    sbig = torch.full((words + 2 * PAD,), GUARD, dtype=torch.int32, device=dev)
    scratch = sbig[PAD:PAD + words]
    scratch.view(torch.uint8).fill_(fill)
    before = prob_d.clone()
    launches = launch_components(C(), [ptr(prob_d), ptr(out), ptr(info), ptr(scratch)], [N, D, H, W, K], thr, largest,
                                 min_size, g, stream())
    torch.cuda.synchronize()
    guard = bool((obig[:PAD] == GUARD).all() and (obig[PAD + n_out:] == GUARD).all() and
                 (ibig[:PAD] == GUARD).all() and (ibig[PAD + N * K * 4:] == GUARD).all() and
                 (sbig[:PAD] == GUARD).all() and (sbig[PAD + words:] == GUARD).all() and torch.equal(before, prob_d))
    return out.clone().view(prob_d.shape), info.view(N, K, 4).clone(), guard, launches


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "K%d-thr%g-%s%s" % (c[0], c[1], "largest" if c[2] else "all",
                                                                           "-min%d" % c[3] if c[3] else ""))
def test_components_kernel_equals_the_oracle(cuda_dev, combo):
    for shape in SHAPES:
        prob, want_out, want_info = _case(shape, combo)
        out, info, guard, _ = _launch(prob.to(cuda_dev), shape, combo)
        cases = [NAMES[_case_id(shape, combo, n, k)] for n in range(shape[0]) for k in range(combo[0])]
        tag = "%s %s %s" % (combo, shape, cases)
        assert guard, tag + ": wrote outside out, info or the scratch, or changed its input"
        assert info.dtype == torch.int32 and out.dtype == torch.float32
        assert torch.equal(info.cpu(), want_info), (tag, info.cpu().tolist(), want_info.tolist())
        assert torch.equal(_bits(out.cpu()), _bits(want_out)), tag       # (bit for bit: -0.0 and 0.0 differ)


def test_forced_situations_are_reached_on_every_shape():
    """The slots of the kernel test hold every situation on every shape, and the oracle sees
    them as what they are meant to be."""
    from unet_distributed_amd.ops.components import labels_torch
    for shape in SHAPES:
        S = int(np.prod(shape[1:]))
        seen = {}
        for combo in COMBOS:
            prob, out, info = _case(shape, combo)
            for n in range(shape[0]):
                for k in range(combo[0]):
                    seen.setdefault(_case_id(shape, combo, n, k), (combo, info[n, k].tolist(), prob[n, ..., k]))
        assert set(seen) == set(range(NCASE)), (shape, sorted(seen))
        D, H, W = shape[1:]
        assert seen[1][1] == [0, 0, 0, 0]                                         # empty
        assert seen[2][1][0] == 1 and seen[2][1][2] == S                          # full: one component of S
        assert seen[3][1][0] == 1 and seen[3][1][2] == 1                          # single voxel
        assert seen[4][1][0] == (S + 1) // 2 and seen[4][1][2] == 1               # checkerboard: all of size 1
        assert seen[5][1][0] == 1 and seen[6][1][0] == 1 and seen[9][1][0] == 1   # serpentine, U, first-to-last
        assert seen[7][1][0] == min(H, W) and seen[7][1][2] == 1                  # diagonal: never connected
        assert seen[8][1][0] == 2 and seen[8][1][2] == 4                          # two equal blobs
        lab = labels_torch(seen[9][2][None, ..., None], seen[9][0][1])
        assert lab.reshape(-1)[0] == 0 and lab.reshape(-1)[-1] == 0               # voxel 0 and voxel S - 1
        assert seen[10][1][0] >= 1                                                # at the threshold: inside


@pytest.mark.parametrize("shape", [(2, 1, 16, 24), (2, 3, 5, CC_SEG + 1)])
def test_two_runs_give_the_same_bits_whatever_the_scratch_held(cuda_dev, shape):
    combo = COMBOS[2]
    prob, want_out, want_info = _case(shape, combo)
    prob_d = prob.to(cuda_dev)
    a, ia, ga, _ = _launch(prob_d, shape, combo, fill=0xFF)
    b, ib, gb, _ = _launch(prob_d, shape, combo, fill=0x00)
    assert ga and gb and torch.equal(_bits(a), _bits(b)) and torch.equal(ia, ib)
    assert torch.equal(ia.cpu(), want_info) and torch.equal(_bits(a.cpu()), _bits(want_out))


def test_sample_groups_give_the_one_group_result(cuda_dev):
    """Five samples in groups of two (a scratch sized for two): three launches, the same bits."""
    from unet_distributed_amd.runtime.executor_base import components_group
    shape, combo = (5, 1, 16, 24), COMBOS[5]
    prob, want_out, want_info = _case(shape, combo)
    prob_d = prob.to(cuda_dev)
    one, info1, g1, l1 = _launch(prob_d, shape, combo)
    two = C().components_scratch(2, 1, 16, 24, combo[0])
    assert components_group(C(), 5, 1, 16, 24, combo[0], cap=two) == 2
    assert components_group(C(), 5, 1, 16, 24, combo[0], cap=1) == 1          # (at least one sample)
    assert components_group(C(), 5, 1, 16, 24, combo[0]) == 5
    split, info2, g2, l2 = _launch(prob_d, shape, combo, group=2)
    assert g1 and g2 and l1 == 1 and l2 == 3
    assert torch.equal(_bits(one), _bits(split)) and torch.equal(info1, info2)
    assert torch.equal(info1.cpu(), want_info) and torch.equal(_bits(one.cpu()), _bits(want_out))


def test_scratch_size_equals_its_mirror_and_refusals_name_the_reason():
    from unet_distributed_amd.runtime.plan_check import components_scratch
    for (N, D, H, W) in SHAPES + [(5, 1, 16, 24), (1, 1, 1, 1), (7, 1, 3, 3)]:
        for K in (1, 2, 3, 4):
            got = C().components_scratch(N, D, H, W, K)
            assert got == components_scratch(N, D, H, W, K) and got % 16 == 0
            assert got >= N * K * (2 * D * H * W + 1 + 5 * -(-(D * H * W) // 16384)) * 4
    assert C().components_check(2, 1, 16, 24, 3, 0) is None
    assert "classes" in C().components_check(2, 1, 16, 24, 5, 0)
    assert "classes" in C().components_check(2, 1, 16, 24, 0, 0)
    assert "min_size" in C().components_check(2, 1, 16, 24, 3, -1)
    assert "S = D H W" in C().components_check(1, 2048, 1024, 1024, 1, 0)
    assert "N S K" in C().components_check(1 << 12, 1024, 1024, 512, 4, 0)
    with pytest.raises(ValueError, match="classes"):
        C().components_scratch(2, 1, 16, 24, 5)
    buf = torch.zeros(16)
    with pytest.raises(ValueError, match="min_size"):
        C().generic("components", [ptr(buf)] * 4, [1, 1, 2, 2, 1, 1, -1], [0.5], 0, 0)


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
    dict(out_channels=2, batch_size=2, img_size=16, in_channels=4, dims=3),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp32"),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=lambda kw: "K%d-%s-%dd" % (kw["out_channels"], kw.get("dtype", "bf16"),
                                                                          kw.get("dims", 2)))
def test_executor_scores_the_filtered_map(cuda_dev, kw):
    """`components`, then `case_stats` / `case_surface` on `prob_pp`, equal the existing oracles
    applied to the oracle's filtered map; `prob` and the plain argument sets are untouched."""
    from unet_distributed_amd.ops.components import components_torch
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    from unet_distributed_amd.runtime.plan_check import check_components_plan
    nb, x, y = _engine(cuda_dev, **kw)
    e = nb.engine
    K, B = kw["out_channels"], kw["batch_size"]
    assert e.prob_pp is None and e.components_scratch is None and e.components_plan is None    # lazily
    with pytest.raises(RuntimeError):
        e.case_stats(0.5, post=True)
    e.load_batch(x, y)
    e.evaluate_batch()
    grid = tuple(e.sdims(1))
    tgt = e.target.view((B,) + grid + (K,)).float().cpu()
    for thr, largest, min_size in ((0.5, True, 0), (0.3, False, 6), (0.5, True, 40)):
        p = e.probs().clone()
        info = e.components(thr, largest, min_size)
        torch.cuda.synchronize()
        assert info.shape == (B, K, 4) and info.dtype == torch.int32
        assert info.data_ptr() == e.components_info.data_ptr()                 # (no allocation per call)
        assert torch.equal(e.probs(), p)                                       # prob is not touched
        want_out, want_info = components_torch(p.cpu(), thr, largest, min_size)
        assert torch.equal(info.cpu(), want_info), (kw, thr, info.cpu().tolist(), want_info.tolist())
        assert torch.equal(_bits(e.probs_pp().cpu()), _bits(want_out))
        surf = e.case_surface(thr, post=True).cpu().long()
        assert torch.equal(surf, case_surface_torch(want_out.view((B,) + grid + (K,)), tgt, thr))
        plain = e.case_surface(thr).cpu().long()
        assert torch.equal(plain, case_surface_torch(p.cpu().view((B,) + grid + (K,)), tgt, thr))
        st = e.case_stats(thr, post=True).double().cpu()
        want_st = case_stats_torch(want_out.view((B,) + grid + (K,)), tgt, thr)
        assert torch.equal(st[..., 3:], want_st[..., 3:].double())             # TP, FP, FN: counts
        assert torch.equal(st[..., 3] + st[..., 4], info.cpu()[..., 3].double())   # TP + FP = kept voxels
    assert check_components_plan(e) == []
    assert e.components_plan.names() == ["components"]
    assert "components" not in e.plan.names() and "components" not in e.eval_plan.names()


def test_native_backend_scores_the_filtered_map_and_pads_a_short_batch(cuda_dev):
    from unet_distributed_amd.ops.components import components_torch
    from unet_distributed_amd.ops.seg_metrics import case_surface_torch
    kw = dict(out_channels=3, batch_size=4, img_size=32, in_channels=4)
    off, x, y = _engine(cuda_dev, **kw)
    nb, _, _ = _engine(cuda_dev, eval_components="largest,min:3", **kw)
    assert off.engine.prob_pp is None and nb.engine.prob_pp is not None      # planned with the flag only
    raw = off.predict(x).cpu()
    want_out, want_info = components_torch(raw, 0.5, True, 3)
    assert torch.equal(_bits(nb.predict(x).cpu()), _bits(want_out))
    info = nb.eval_components(x, y, 0.5).cpu()
    assert torch.equal(info, want_info)
    short = nb.eval_components(x[:3], y[:3], 0.5).cpu()
    assert short.shape == (3, 3, 4) and torch.equal(short, info[:3])
    surf = nb.eval_surface(x[:3], y[:3], 0.5).cpu().long()
    assert torch.equal(surf, case_surface_torch(want_out[:3], y[:3].float().cpu(), 0.5))
    st = nb.eval_stats(x[:3], y[:3], 0.5).cpu()
    assert torch.equal(st[..., 3] + st[..., 4], info[:3, :, 3].float())
    sums_on, sums_off = nb.eval_sums(x, y).cpu(), off.eval_sums(x, y).cpu()
    assert torch.equal(sums_on, sums_off)                                     # the pooled sums never see the filter
    assert torch.equal(nb.last_eval_components(0.5).cpu(), want_info)
    assert torch.equal(nb.last_eval_surface(0.5).cpu().long(), case_surface_torch(want_out, y.float().cpu(), 0.5))
    with pytest.raises(RuntimeError, match="eval_components"):
        off.last_eval_components(0.5)


# ------------------------------------------------------------------ trainer
def _trainer_cfg(tmp_path, **kw):
    from unet_distributed_amd.config import Config
    return Config(synthetic=True, synthetic_train=8, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                  device="cuda", checkpoint_dir=str(tmp_path), no_checkpoint=True, tensorboard=False, export=False,
                  resume=False, progress=False, eval_hd95=True, **kw)


def test_trainer_evaluate_native_against_torch(cuda_dev, tmp_path):
    """--eval_components largest --eval_hd95: the integer-derived fields of the HIP path equal the
    same run on --backend torch (fp32 on both, the one precision the two share)."""
    from unet_distributed_amd.runtime.trainer import Trainer
    got = {}
    for backend in ("native", "torch"):
        tr = Trainer(_trainer_cfg(tmp_path, backend=backend, dtype="fp32", eval_components="largest"))
        assert tr.backend.name == backend
        got[backend] = tr.evaluate()
    a, b = got["native"], got["torch"]
    assert a["components"] == b["components"] == "largest"
    assert a["batches"] == b["batches"] == 2 and a["cases"] == b["cases"] == 10
    assert a["per_class"]["components"] == b["per_class"]["components"]
    assert a["per_class"]["components_kept"] == b["per_class"]["components_kept"]
    for k in ("case_dice", "sensitivity", "specificity", "hd95"):           # from true counts and distances
        assert a["per_class"][k] == b["per_class"][k], k
    assert a["case_dice"] == b["case_dice"] and a["hd95"] == b["hd95"]
    assert all(0.0 <= v <= 1.0 for v in a["per_class"]["components_kept"])
    assert set(a["per_class"]) == set(b["per_class"]) == {"dice", "case_dice", "sensitivity", "specificity", "hd95",
                                                           "components", "components_kept"}


def test_trainer_evaluate_scores_the_filtered_map(cuda_dev, tmp_path):
    """Multi-class bf16: every per-case field equals the oracles applied to the oracle's filter
    of the unfiltered predictions (two full batches and a padded tail of 2); the pooled block is
    that of the run with the option off."""
    from unet_distributed_amd.ops import seg_metrics
    from unet_distributed_amd.ops.components import components_torch
    from unet_distributed_amd.runtime.trainer import Trainer
    off = Trainer(_trainer_cfg(tmp_path, backend="native", out_channels=3))
    tr = Trainer(_trainer_cfg(tmp_path, backend="native", out_channels=3, eval_components="largest,min:2"))
    assert off.backend.engine.prob_pp is None and tr.backend.engine.prob_pp is not None
    m0, m = off.evaluate(), tr.evaluate()
    assert "components" not in m0 and "components" not in m0["per_class"]
    for k in ("loss", "dice", "sensitivity", "specificity", "batches"):
        assert m[k] == m0[k], k
    probs = []
    for s in (0, 4, 8):
        xb = torch.from_numpy(np.ascontiguousarray(off.x_test[s:s + 4])).to(cuda_dev)
        n = xb.shape[0]
        if n < 4:
            xb = torch.cat([xb, xb.new_zeros((4 - n,) + tuple(xb.shape[1:]))])
        probs.append(off.backend.predict(xb)[:n].cpu())
    out, info = components_torch(torch.cat(probs), 0.5, True, 2)
    y = torch.from_numpy(off.y_test).float()
    want_hd = seg_metrics.hd95_from_surface(seg_metrics.case_surface_torch(out, y, 0.5), (32, 32)).mean(0)
    assert np.allclose(m["per_class"]["hd95"], want_hd, rtol=0, atol=1e-9)
    hm = seg_metrics.metrics_from_case_stats(seg_metrics.case_stats_torch(out, y, 0.5).numpy(), 32 * 32)
    assert np.allclose(m["per_class"]["case_dice"], hm["case_dice"], rtol=0, atol=1e-9)
    assert m["per_class"]["components"] == info[..., 0].double().mean(0).tolist()
    assert m["per_class"]["components_kept"] == info[..., 1].double().mean(0).tolist()
    assert m["components"] == "largest,min:2" and m["cases"] == 10


# ------------------------------------------------------------------ inference
def test_predictor_returns_the_filtered_map(cuda_dev, tmp_path):
    """Predictor(components=...) on the native backend: `predict` (6 samples at batch 4) and
    `predict_sliding` on 40x56 images with the 32 tile equal the oracle applied to the
    unfiltered result; `components` / `components_sliding` give its info."""
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.ops.components import components_torch
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=3, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    path = export_model(cfg, spec, flat)
    plain = load_saved_model(path, device=cuda_dev, batch=4)
    model = load_saved_model(path, device=cuda_dev, batch=4, components="largest")
    assert model.name == "native" and plain.name == "native"
    x, _ = synthetic_brats(6, 32, 4, seed=2, out_channels=3)
    want_out, want_info = components_torch(torch.from_numpy(plain.predict(x)), 0.5, True, 0)
    assert np.array_equal(model.predict(x).view(np.int32), want_out.numpy().view(np.int32))
    got = model.components(x)
    assert got.shape == (6, 3, 4) and got.dtype == np.int64 and np.array_equal(got, want_info.long().numpy())
    rng = np.random.RandomState(4)
    big = rng.randn(2, 40, 56, 4).astype(np.float32)
    want_out, want_info = components_torch(torch.from_numpy(plain.predict_sliding(big)), 0.5, True, 0)
    assert np.array_equal(model.predict_sliding(big).view(np.int32), want_out.numpy().view(np.int32))
    assert np.array_equal(model.components_sliding(big), want_info.long().numpy())
    with pytest.raises(RuntimeError, match="components"):
        plain.components(x)

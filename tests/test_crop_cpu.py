"""Patch-sampled training off the GPU: the --crop flags, the foreground table, the
counter-based origin draw (data/augment.py draw_crop), crop_torch against numpy indexing,
the streamed feeder, plan-time validation of the gather_batch_crop ops on the CPU dry run,
and the trainer on the ATen backend (patches in, sliding-window evaluation out)."""
import numpy as np
import pytest
import torch

from unet_distributed_amd.data import augment as A
from unet_distributed_amd.data import datasets


# ------------------------------------------------------------------ flags
def test_crop_flags_default_off_and_validated():
    from unet_distributed_amd.config import Config, parse_args, parse_crop, validate
    c = Config()
    assert c.crop == "" and c.synthetic_size == 0 and c.eval_overlap == 0.5 and c.eval_blend == "gaussian"
    assert parse_crop("") == ("", 0.0) and parse_crop("random") == ("random", 0.0)
    assert parse_crop("foreground") == ("foreground", 1.0 / 3.0)
    assert parse_crop("foreground:0.5") == ("foreground", 0.5) and parse_crop(" foreground:1 ") == ("foreground", 1.0)
    cfg = parse_args(["--crop", "foreground:0.25", "--synthetic_size", "240", "--eval_overlap", "0.25",
                      "--eval_blend", "constant"])
    assert parse_crop(cfg.crop) == ("foreground", 0.25) and cfg.synthetic_size == 240
    assert cfg.eval_overlap == 0.25 and cfg.eval_blend == "constant"
    for bad, item in (("foreground:0", "foreground:0"), ("foreground:1.5", "foreground:1.5"), ("centre", "centre"),
                      ("random,random", "random"), ("random,foreground", "foreground"), ("foreground:x", "foreground:x"),
                      ("foreground:nan", "foreground:nan"), ("random:0.5", "random:0.5"), ("foreground:", "foreground:"),
                      ("Random", "Random")):
        with pytest.raises(SystemExit) as e:
            parse_args(["--crop", bad])
        assert item in str(e.value), (bad, str(e.value))
    for kw in (dict(eval_overlap=0.9), dict(eval_overlap=-0.1), dict(eval_overlap=float("nan")),
               dict(eval_blend="linear"), dict(synthetic_size=-1), dict(crop="centre")):
        with pytest.raises(SystemExit):
            validate(Config(**kw))
    validate(Config(crop="foreground:1", eval_overlap=0.75, synthetic_size=240))


# ------------------------------------------------------------------ foreground table
def _brute_table(y, R):
    fg = np.full((len(y), R), -1, dtype=np.int64)
    cnt = np.zeros(len(y), dtype=np.int64)
    for i in range(len(y)):
        L = [lin for lin, v in enumerate(y[i].reshape(-1, y.shape[-1])) if (v >= 0.5).any()]
        n = cnt[i] = len(L)
        for j in range(min(n, R)):
            fg[i, j] = L[j] if n <= R else L[((2 * j + 1) * n) // (2 * R)]
    return fg, cnt


def test_foreground_table_matches_a_brute_force_listing():
    rng = np.random.default_rng(0)
    R = 8
    y = np.zeros((6, 5, 7, 2), dtype=np.float32)
    flat = y.reshape(6, 35, 2)
    for i, n in enumerate((0, 3, 8, 9, 20, 35)):           # n = 0, n < R, n = R, n > R (just, well, all)
        pos = rng.permutation(35)[:n]
        flat[i, pos, rng.integers(0, 2, size=n)] = rng.uniform(0.5, 1.0, size=n).astype(np.float32)
    flat[1, :, 0] = np.where(flat[1, :, 0] == 0, 0.49, flat[1, :, 0])      # (below the threshold: background)
    fg, cnt = datasets.foreground_table(y, R)
    bf, bc = _brute_table(y, R)
    assert fg.dtype == np.int32 and cnt.dtype == np.int32 and fg.shape == (6, R)
    assert cnt.tolist() == [0, 3, 8, 9, 20, 35] == bc.tolist() and np.array_equal(fg, bf)
    assert (fg[0] == -1).all() and (fg[1, 3:] == -1).all() and (fg[2:] >= 0).all()
    for row in fg[1:]:
        v = row[row >= 0]
        assert (np.diff(v) > 0).all()                       # ascending, no entry twice
    # 3D and the default R
    y3 = (rng.random((2, 4, 6, 5, 1)) > 0.5).astype(np.float32)
    f3, c3 = datasets.foreground_table(y3)
    b3, bc3 = _brute_table(y3, 32)
    assert f3.shape == (2, 32) and np.array_equal(f3, b3) and np.array_equal(c3, bc3)
    assert np.array_equal(datasets.foreground_table(y3)[0], f3)            # no RNG


# ------------------------------------------------------------------ draw_crop
def _targets(n, S, seed=0, empty=()):
    """Targets [n][Hs][Ws][1] with one small foreground square each (none for `empty`)."""
    rng = np.random.default_rng(seed)
    y = np.zeros((n,) + tuple(S) + (1,), dtype=np.float32)
    for i in range(n):
        if i in empty:
            continue
        h, w = rng.integers(0, S[0] - 3), rng.integers(0, S[1] - 3)
        y[i, h:h + 3, w:w + 3, 0] = 1
    return y


def test_draw_crop_depends_only_on_seed_step_and_sample_index():
    S, T = (1, 40, 56), (1, 16, 16)
    y = _targets(64, S[1:])
    table = datasets.foreground_table(y)
    idx = np.arange(64)
    for mode, p in (("random", 0.0), ("foreground", 0.5)):
        org, used = A.draw_crop(816, 7, idx, S, T, mode, p, table)
        assert org.dtype == np.int32 and org.shape == (64, 3) and used.dtype == bool and used.shape == (64,)
        again = A.draw_crop(816, 7, idx, S, T, mode, p, table)
        assert np.array_equal(again[0], org) and np.array_equal(again[1], used)             # deterministic
        perm = np.random.default_rng(1).permutation(64)
        o2, u2 = A.draw_crop(816, 7, idx[perm], S, T, mode, p, table)
        assert np.array_equal(o2, org[perm]) and np.array_equal(u2, used[perm])             # batch order
        # two shards of the batch (DP = 2): each rank draws its own half
        oa, ob = (A.draw_crop(816, 7, part, S, T, mode, p, table)[0] for part in (idx[:32], idx[32:]))
        assert np.array_equal(np.concatenate([oa, ob]), org)
        for other in (A.draw_crop(816, 8, idx, S, T, mode, p, table), A.draw_crop(817, 7, idx, S, T, mode, p, table)):
            assert (other[0] != org).any(axis=1).mean() > 0.5                               # other steps, seeds
        assert (org >= 0).all() and (org <= np.array(S) - np.array(T)).all() and (org[:, 0] == 0).all()
        assert (used.any() and not used.all()) if mode == "foreground" else not used.any()
        # (H, W) sizes are (1, H, W)
        assert np.array_equal(A.draw_crop(816, 7, idx, S[1:], T[1:], mode, p, table)[0], org)
    # uniform origins reach both ends of every free axis
    org = np.concatenate([A.draw_crop(1, s, idx, S, T, "random")[0] for s in range(20)])
    assert org[:, 1].min() == 0 and org[:, 1].max() == 24 and org[:, 2].min() == 0 and org[:, 2].max() == 40
    # 3D: every axis is drawn
    o3 = A.draw_crop(1, 2, idx, (20, 24, 28), (16, 16, 16), "random")[0]
    assert (o3 >= 0).all() and (o3 <= np.array([4, 8, 12])).all() and all(len(np.unique(o3[:, a])) > 2 for a in range(3))
    # stored == patch: every origin is 0
    assert not A.draw_crop(1, 2, idx, T, T, "random")[0].any()
    assert not A.draw_crop(1, 2, idx, (1, 56, 56), (1, 56, 56), "foreground", 1.0,
                           datasets.foreground_table(_targets(64, (56, 56))))[0].any()
    with pytest.raises(ValueError):
        A.draw_crop(1, 2, idx, (1, 16, 16), (1, 32, 32), "random")
    with pytest.raises(ValueError):
        A.draw_crop(1, 2, idx, S, T, "centre")
    with pytest.raises(ValueError):
        A.draw_crop(1, 2, idx, S, T, "foreground", 0.5)                                     # no table


def test_foreground_patches_contain_foreground():
    S, T = (40, 56), (16, 16)
    empty = (3, 10)
    y = _targets(24, S, seed=2, empty=empty)
    x = np.zeros(y.shape[:-1] + (1,), dtype=np.float32)
    table = datasets.foreground_table(y)
    assert all(table[1][i] == 0 for i in empty)
    idx = np.arange(24)
    seen_empty = []
    for step in range(6):
        org, used = A.draw_crop(5, step, idx, S, T, "foreground", 1.0, table)
        _, ty = A.crop_torch(torch.from_numpy(x), torch.from_numpy(y), org, T)
        has = ty.flatten(1).sum(dim=1) > 0
        for i in range(24):
            assert used[i] == (i not in empty)
            if i not in empty:
                assert has[i], (step, i, org[i])
        uni = A.draw_crop(5, step, idx, S, T, "random")[0]
        assert np.array_equal(org[list(empty)], uni[list(empty)])          # cnt = 0: the uniform rule
        seen_empty.append(org[list(empty)])
    assert len(np.unique(np.concatenate(seen_empty), axis=0)) > 2
    # the patch holds the drawn voxel even at the borders: foreground in the corners, 3D too
    y3 = np.zeros((2, 20, 24, 28, 1), dtype=np.float32)
    y3[0, 0, 0, 0] = y3[1, 19, 23, 27] = 1
    t3 = datasets.foreground_table(y3)
    o3, u3 = A.draw_crop(1, 1, [0, 1], (20, 24, 28), (16, 16, 16), "foreground", 1.0, t3)
    assert u3.all() and o3.tolist() == [[0, 0, 0], [4, 8, 12]]


def test_foreground_share_is_the_probability():
    """P = 1/3 over 4096 (step, sample) pairs that all have foreground: the share of forced
    patches is binomial, sigma = sqrt(P (1 - P) / 4096) = 0.0074; 4 sigma = 0.03."""
    y = _targets(64, (40, 56), seed=3)
    table = datasets.foreground_table(y)
    used = np.concatenate([A.draw_crop(816, step, np.arange(64), (40, 56), (16, 16), "foreground", 1.0 / 3.0, table)[1]
                           for step in range(64)])
    assert used.shape == (4096,) and abs(used.mean() - 1.0 / 3.0) <= 0.03, used.mean()


def test_draw_is_the_same_with_and_without_crop():
    from unet_distributed_amd.config import Config
    idx = np.arange(50, 90)
    plain = Config(augment="flip,rot90,intensity", in_channels=4, img_size=32)
    crop = Config(augment="flip,rot90,intensity", in_channels=4, img_size=32, crop="foreground")
    table = datasets.foreground_table(_targets(90, (48, 48)))
    for step in (0, 3):
        c0, a0 = A.make_aug(plain, step)(idx)
        c1, a1, org = A.make_crop_aug(crop, step, (1, 48, 48), table)(idx)
        assert np.array_equal(c0, c1) and np.array_equal(a0, a1) and org.shape == (40, 3)
        assert np.array_equal(org, A.draw_crop(crop.seed, step, idx, (48, 48), (32, 32), "foreground", 1 / 3, table)[0])
    # without --augment: zero codes, no affine, the same origins
    c2, a2, o2 = A.make_crop_aug(Config(in_channels=4, img_size=32, crop="foreground"), 3, (1, 48, 48), table)(idx)
    assert not c2.any() and c2.dtype == np.int32 and a2 is None and np.array_equal(o2, org)
    # draw's values themselves are pinned (seed 816, step 7, samples 100..103)
    code, aff = A.draw(816, 7, np.arange(100, 104), "flip,rot90,intensity", 1, 2, 0.1)
    again = A.draw(816, 7, np.arange(100, 104), "flip,rot90,intensity", 1, 2, 0.1)
    assert np.array_equal(code, again[0]) and np.array_equal(aff, again[1])


# ------------------------------------------------------------------ crop_torch
def test_crop_then_apply_matches_numpy_indexing():
    rng = np.random.default_rng(5)
    # 2D: stored 12 x 14, patch 8; every code
    x = rng.standard_normal((8, 12, 14, 3)).astype(np.float32)
    y = (rng.random((8, 12, 14, 2)) > 0.5).astype(np.float32)
    org = np.stack([np.zeros(8, int), rng.integers(0, 5, 8), rng.integers(0, 7, 8)], axis=1)
    org[0], org[1] = (0, 0, 0), (0, 4, 6)
    code = np.arange(8)
    aff = np.stack([rng.uniform(0.8, 1.2, (8, 3)), rng.uniform(-0.2, 0.2, (8, 3))], axis=-1).astype(np.float32)
    cx, cy = A.crop_torch(torch.from_numpy(x), torch.from_numpy(y), org, (8, 8))
    gx, gy = A.apply_torch(cx, cy, code, aff)
    T = 8
    for n in range(8):
        for h in range(T):
            for w in range(T):
                a, b = (w, h) if code[n] & A.T else (h, w)
                hh = T - 1 - a if code[n] & A.FH else a
                ww = T - 1 - b if code[n] & A.FW else b
                src = x[n, org[n, 1] + hh, org[n, 2] + ww]
                want = (src.astype(np.float64) * aff[n, :, 0] + aff[n, :, 1]).astype(np.float32)
                assert np.array_equal(gx[n, h, w].numpy(), want)
                assert np.array_equal(gy[n, h, w].numpy(), y[n, org[n, 1] + hh, org[n, 2] + ww])
    assert cx.shape == (8, 8, 8, 3) and np.array_equal(cx[1].numpy(), x[1, 4:12, 6:14])
    # 3D: stored 6 x 7 x 9, patch 4; every code
    x3 = rng.standard_normal((16, 6, 7, 9, 2)).astype(np.float32)
    y3 = (rng.random((16, 6, 7, 9, 1)) > 0.5).astype(np.float32)
    o3 = np.stack([rng.integers(0, 3, 16), rng.integers(0, 4, 16), rng.integers(0, 6, 16)], axis=1)
    o3[5] = (2, 3, 5)
    c3 = np.arange(16)
    gx3, gy3 = A.apply_torch(*A.crop_torch(torch.from_numpy(x3), torch.from_numpy(y3), o3, (4, 4, 4)), c3)
    T = 4
    want_x, want_y = np.empty((16, 4, 4, 4, 2), np.float32), np.empty((16, 4, 4, 4, 1), np.float32)
    for n in range(16):
        for d in range(T):
            for h in range(T):
                for w in range(T):
                    a, b = (w, h) if c3[n] & A.T else (h, w)
                    pos = (n, o3[n, 0] + (T - 1 - d if c3[n] & A.FD else d),
                           o3[n, 1] + (T - 1 - a if c3[n] & A.FH else a), o3[n, 2] + (T - 1 - b if c3[n] & A.FW else b))
                    want_x[n, d, h, w], want_y[n, d, h, w] = x3[pos], y3[pos]
    assert np.array_equal(gx3.numpy(), want_x) and np.array_equal(gy3.numpy(), want_y)
    # origins outside the sample, a wrong count, a 3D patch of 2D samples
    for bad in ([[0, 5, 0]] * 8, [[0, 0, -1]] * 8, [[0, 0, 0]] * 7, [[1, 0, 0]] * 8):
        with pytest.raises(ValueError):
            A.crop_torch(torch.from_numpy(x), torch.from_numpy(y), np.array(bad), (8, 8))
    with pytest.raises(ValueError):
        A.crop_torch(torch.from_numpy(x), torch.from_numpy(y), np.zeros((8, 3), int), (2, 8, 8))


# ------------------------------------------------------------------ feeder
@pytest.mark.parametrize("dims", [2, 3])
def test_streamed_feeder_crops_on_the_host_into_patch_sized_buffers(dims):
    from unet_distributed_amd.data.loader import DeviceFeeder, ResidentBatch
    rng = np.random.default_rng(4)
    S = (24, 28) if dims == 2 else (10, 12, 14)
    patch = (1, 16, 16) if dims == 2 else (8, 8, 8)
    x = rng.standard_normal((11,) + S + (4,)).astype(np.float32)
    y = (rng.random((11,) + S + (3,)) < 0.3).astype(np.float32)
    table = datasets.foreground_table(y)
    f = DeviceFeeder(x, y, 4, "cpu", patch=patch)
    assert not f.resident
    for ld in f.loaders:
        assert tuple(ld.bx.shape) == (4,) + patch[3 - dims:] + (4,) and tuple(ld.by.shape) == (4,) + patch[3 - dims:] + (3,)
    idx = np.array([9, 2, 7, 2])
    si = np.sort(idx)
    seen = []

    def aug(sorted_idx):
        seen.append(np.array(sorted_idx))
        code, aff = A.draw(1, 2, sorted_idx, "flip,rot90,intensity", 4, dims, 0.2)
        return code, aff, A.draw_crop(1, 2, sorted_idx, (1,) * (3 - dims) + S, patch, "foreground", 0.5, table)[0]

    gx, gy = f.get(idx, aug=aug)
    assert len(seen) == 1 and np.array_equal(seen[0], si)
    code, aff, org = aug(si)
    wx, wy = A.apply_torch(*A.crop_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch), code, aff)
    assert torch.equal(gx, wx) and torch.equal(gy, wy) and tuple(gx.shape) == (4,) + patch[3 - dims:] + (4,)
    assert gx[0].equal(gx[1])                               # the repeated sample: same origin, same pixels
    # origins alone (no --augment): the plain patches
    px, py = f.get(idx, aug=lambda s: (np.zeros(len(s), np.int32), None, org))
    cx, cy = A.crop_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch)
    assert torch.equal(px, cx) and torch.equal(py, cy)
    with pytest.raises(ValueError):
        f.get(idx)                                          # a cropping feeder needs the origins
    # a ResidentBatch hands out the same batch and counts patch pixels
    rb = ResidentBatch(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(si),
                       (torch.from_numpy(code), torch.from_numpy(aff)), (torch.from_numpy(org), patch))
    tx, ty = rb.tensors()
    assert torch.equal(tx, wx) and torch.equal(ty, wy) and rb.npix == 4 * int(np.prod(patch)) * 3
    # a feeder without a patch is what it was
    g0 = DeviceFeeder(x, y, 4, "cpu").get(idx)
    assert np.array_equal(g0[0].numpy(), x[si]) and np.array_equal(g0[1].numpy(), y[si])


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


@pytest.mark.parametrize("kind", ["gather_batch_crop", "f32_gather_batch_crop"])
def test_gather_batch_crop_plan_time_validation(kind):
    C = _C()
    for dt in ((0, 1) if kind == "gather_batch_crop" else (0,)):
        plan = C.Plan(dt)
        ptrs = [4096 * (i + 1) for i in range(8)]
        # ints: B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K
        for ints in ([8, 1, 56, 40, 1, 32, 32, 4, 4, 3], [16, 20, 24, 28, 16, 16, 16, 4, 4, 2],
                     [2, 1, 16, 16, 1, 16, 16, 1, 4, 1], [4, 1, 240, 240, 1, 32, 32, 8, 8, 4],
                     [2, 1, 40, 56, 1, 16, 16, 3, 32, 1], [1024, 1, 240, 240, 1, 128, 128, 4, 4, 1],
                     [8, 155, 240, 240, 128, 128, 128, 4, 4, 1]):
            i = plan.add_generic(kind, ptrs, ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
            i = plan.add_generic(kind, ptrs[:4] + [0, 0] + ptrs[6:], ints, [], "gather")       # null code and affine
            assert plan.check_dispatch(i, i + 1) == []
        n0 = plan.size()
        bad = ([2, 1, 48, 48, 1, 32, 16, 4, 4, 1],             # H != W
               [2, 1, 31, 48, 1, 32, 32, 4, 4, 1], [2, 1, 48, 31, 1, 32, 32, 4, 4, 1],      # patch > stored
               [2, 8, 48, 48, 16, 32, 32, 4, 4, 1],
               [2, 1, 48, 48, 1, 32, 32, 4, 4, 5], [2, 1, 48, 48, 1, 32, 32, 4, 4, 0],      # K outside 1..4
               [2, 1, 48, 48, 1, 32, 32, 8, 4, 1], [2, 1, 48, 48, 1, 32, 32, 4, 128, 1],    # Cin <= Cpad <= 64
               [2, 1, 48, 48, 1, 32, 32, 0, 4, 1],
               [2, 1, 48, 48, 0, 32, 32, 4, 4, 1], [0, 1, 48, 48, 1, 32, 32, 4, 4, 1],      # D, B >= 1
               [2, 1, 1 << 20, 48, 1, 32, 32, 4, 4, 1],                                      # stored side
               [1024, 1, 512, 512, 1, 512, 512, 8, 8, 1], [1 << 40, 1 << 19, 1, 1, 1 << 19, 1, 1, 1, 1, 1])  # >= 2^31
        for ints in bad:
            with pytest.raises(ValueError) as e:
                plan.add_generic(kind, ptrs, ints, [], "gather")
            assert "gather_batch_crop" in str(e.value)
            with pytest.raises(ValueError):
                C.generic(kind, ptrs, ints, [], 0, dt)                   # (immediate style: nothing launched)
        good = [2, 1, 48, 48, 1, 32, 32, 4, 4, 1]
        for missing in (0, 1, 2, 3, 6, 7):          # every pointer but the code and the affine is required
            with pytest.raises(ValueError):
                plan.add_generic(kind, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs[:7], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, good[:9], [], "")
        assert plan.size() == n0


def test_plan_check_knows_the_extents_of_the_crop_ops():
    from unet_distributed_amd.runtime.plan_check import _generic_rw, _generic_write_spans
    p = [4096 * (i + 1) for i in range(8)]
    ints = [8, 5, 40, 56, 2, 16, 16, 3, 4, 2]
    px = 8 * 2 * 16 * 16                            # patch pixels: the stored size does not enter
    assert _generic_write_spans("gather_batch_crop", p, ints) == [(p[6], px * 4 * 2), (p[7], px * 2 * 2)]
    assert _generic_write_spans("f32_gather_batch_crop", p, ints) == [(p[6], px * 4 * 4), (p[7], px * 2 * 4)]
    assert _generic_rw("gather_batch_crop", p, ints) == (p[:6], p[6:])
    assert _generic_rw("f32_gather_batch_crop", p[:4] + [0, 0] + p[6:], ints) == (p[:4], p[6:])


# ------------------------------------------------------------------ trainer on the ATen backend
def _trainer_cfg(tmp, **kw):
    from unet_distributed_amd.config import Config
    base = dict(synthetic=True, synthetic_train=16, synthetic_test=10, batch_size=4, img_size=32, in_channels=4,
                out_channels=1, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False, steps=2,
                log_every=1000)
    return Config(**dict(base, **kw))


def _record(tr):
    fed = {}
    inner = tr.backend.fwd_bwd

    def fwd_bwd(x, y, seed, **kw):
        fed[tr.flat.global_step] = (x.clone(), y.clone())
        return inner(x, y, seed, **kw)

    tr.backend.fwd_bwd = fwd_bwd
    return fed


def test_cpu_trainer_trains_on_patches_and_evaluates_through_sliding_windows(tmp_path, capsys):
    from unet_distributed_amd.ops import seg_metrics
    from unet_distributed_amd.runtime.trainer import Trainer, metrics_from_sums
    tr = Trainer(_trainer_cfg(tmp_path, synthetic_size=48, crop="foreground", eval_hd95=True))
    out = capsys.readouterr().out
    assert "Training patches: 32 x 32 of 48 x 48, foreground 0.33\n" in out
    assert "Evaluation: sliding window, overlap 0.5, gaussian\n" in out
    assert tr.x_train.shape == (16, 48, 48, 4) and tr.x_test.shape == (10, 48, 48, 4)
    fed = _record(tr)
    res = tr.run()
    assert res["global_step"] == 2 and np.isfinite(res["train"]["loss"]) and sorted(fed) == [0, 1]
    table = datasets.foreground_table(tr.y_train)
    epoch = tr.sampler.epoch_indices(0)
    for step in range(2):
        si = np.sort(epoch[step])
        org, _ = A.draw_crop(tr.cfg.seed, step, si, (48, 48), (32, 32), "foreground", 1.0 / 3.0, table)
        wx, wy = A.crop_torch(torch.from_numpy(tr.x_train[si]), torch.from_numpy(tr.y_train[si]), org, (32, 32))
        assert torch.equal(fed[step][0], wx) and torch.equal(fed[step][1], wy) and tuple(wx.shape) == (4, 32, 32, 4)
    # the evaluation == a direct composition of predict_sliding + sliding_stats on the same weights
    m = res["test"]
    assert m["sliding"] == {"overlap": 0.5, "blend": "gaussian"} and m["cases"] == 10 and m["batches"] == 2
    assert m == tr.evaluate()
    be, B = tr.backend, 4
    pooled, soft, stats_all, hd = [], [], [], []
    for lo in (0, 4, 8):
        x, y = torch.from_numpy(tr.x_test[lo:lo + B]), torch.from_numpy(tr.y_test[lo:lo + B])
        p = be.predict_sliding(x, 0.5, "gaussian")
        st = be.sliding_stats(p, y, 0.5)
        stats_all.append(st)
        hd.append(seg_metrics.accumulate_hd95(be.sliding_surface(p, y, 0.5), (48, 48))["hd95_sum"])
        if len(x) == B:
            s = st[..., :3].double().sum(dim=(0, 1))
            bce = torch.nn.functional.binary_cross_entropy(p, y, reduction="sum").double().reshape(1)
            pooled.append(metrics_from_sums(torch.cat([s, bce]), y.numel(), tr.cfg))
            soft.append(seg_metrics.soft_dice(st))
    for k in ("loss", "dice", "sensitivity", "specificity"):
        assert m[k] == pytest.approx(np.mean([q[k] for q in pooled]), rel=1e-12, abs=1e-12), k
    assert m["per_class"]["dice"] == pytest.approx(np.mean(soft, axis=0).tolist(), rel=1e-12)
    hm = seg_metrics.hard_metrics(seg_metrics.accumulate(torch.cat(stats_all), 48 * 48))
    for k in ("case_dice", "sensitivity", "specificity"):
        assert m["per_class"][k] == pytest.approx(hm[k], rel=1e-12, nan_ok=True), k
    assert m["case_dice"] == pytest.approx(hm["case_dice_mean"], rel=1e-12)
    assert m["per_class"]["hd95"] == pytest.approx((np.sum(hd, axis=0) / 10).tolist(), rel=1e-12)


def test_cpu_trainer_sliding_evaluation_with_components_and_tta(tmp_path):
    """--eval_components: the per-class lines are of the filtered map, the pooled block of the
    un-filtered one; --eval_tta rides inside predict_sliding."""
    from unet_distributed_amd.runtime.trainer import Trainer, metrics_from_sums
    kw = dict(synthetic_size=48, crop="random", eval_tta="flip", steps=1)
    tr = Trainer(_trainer_cfg(tmp_path / "a", eval_components="largest", **kw))
    plain = Trainer(_trainer_cfg(tmp_path / "b", **kw))
    assert torch.equal(tr.flat.master, plain.flat.master)
    m, m0 = tr.evaluate(), plain.evaluate()
    for k in ("loss", "dice", "sensitivity", "specificity"):
        assert m[k] == m0[k], k                                # pooled: un-filtered
    assert m["components"] == "largest" and m["tta"] == 4 and "components" in m["per_class"]
    assert m["per_class"]["components_kept"] == [1.0] and m["per_class"]["components"][0] >= 1.0
    assert m["sliding"] == m0["sliding"] and "components" not in m0
    be = tr.backend
    x, y = torch.from_numpy(tr.x_test[:4]), torch.from_numpy(tr.y_test[:4])
    raw = be.predict_sliding(x, 0.5, "gaussian", post=False)
    assert torch.equal(raw, plain.backend.predict_sliding(x, 0.5, "gaussian"))
    assert torch.equal(be.sliding_filter(raw, 0.5), be.predict_sliding(x, 0.5, "gaussian"))
    assert torch.equal(be.sliding_stats(raw, y, 0.5, post=False), plain.backend.sliding_stats(raw, y, 0.5))


def test_cpu_trainer_refuses_a_size_mismatch_without_crop(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    with pytest.raises(SystemExit) as e:
        Trainer(_trainer_cfg(tmp_path, synthetic_size=48))
    assert "48 x 48" in str(e.value) and "32 x 32" in str(e.value) and "--crop" in str(e.value)
    with pytest.raises(SystemExit) as e:
        Trainer(_trainer_cfg(tmp_path, synthetic_size=16, crop="random"))
    assert "16 x 16" in str(e.value) and "32 x 32" in str(e.value) and "smaller" in str(e.value)


def test_cpu_trainer_crop_of_the_stored_size_is_the_uncropped_run(tmp_path, capsys):
    from unet_distributed_amd.runtime.trainer import Trainer
    a = Trainer(_trainer_cfg(tmp_path / "a", synthetic_size=32, crop="random"))
    assert "Training patches: 32 x 32 of 32 x 32, uniform\n" in capsys.readouterr().out and not a.eval_sliding
    b = Trainer(_trainer_cfg(tmp_path / "b"))
    ra, rb = a.run(), b.run()
    assert ra["train"]["loss"] == rb["train"]["loss"] and torch.equal(a.flat.master, b.flat.master)
    assert ra["test"] == rb["test"] and "sliding" not in ra["test"]

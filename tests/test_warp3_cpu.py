"""--augment rotate3d,scale3d without a GPU: draw_spatial3 (the 3 x 3 matrices, their hash lanes and
the embedding of draw_spatial's integers), warp3_torch (the definition gather_batch_warp3 is held
to) against warp_torch / elastic_torch where the matrix leaves depth alone and against exact
permutations, flips and half-voxel shifts where it does not, the refusals of validate, the item
shapes of make_aug / make_crop_aug, the streamed feeder, the trainer's log, and the plan-time
validation of the op.
"""
import json

import numpy as np
import pytest
import torch

from unet_distributed_amd import config
from unet_distributed_amd.data import augment as A

ONE = 65536


def _data(stored, cin, K, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n,) + tuple(stored) + (cin,), generator=g)
    y = (torch.rand((n,) + tuple(stored) + (K,), generator=g) > 0.6).float()
    return x, y


# ------------------------------------------------------------------ draw_spatial3
@pytest.mark.parametrize("names", ["rotate,scale", "rotate", "scale", "flip,rot90"])
def test_in_plane_names_embed_draw_spatial(names):
    idx = np.arange(64) * 7 + 1
    for step in (0, 11):
        m2 = A.draw_spatial(5, step, idx, names, 40.0, 0.5)
        m3 = A.draw_spatial3(5, step, idx, names, 40.0, 15.0, 0.5)
        assert m3.dtype == np.int32 and m3.shape == (64, 9)
        assert np.array_equal(m3[:, [4, 5, 7, 8]], m2)
        assert np.array_equal(m3[:, :3], np.tile([ONE, 0, 0], (64, 1))) and (m3[:, [3, 6]] == 0).all()
        assert np.array_equal(A.embed_mat3(m2), m3)


def test_a_3d_name_changes_no_other_drawn_parameter():
    idx = np.array([3, 9, 10, 250, 7])
    base, more = "flip,rot90,intensity,rotate,scale,elastic", "flip,rot90,intensity,rotate3d,scale3d,elastic"
    for a, b in zip(A.draw(2, 4, idx, base, 4, 3, 0.2), A.draw(2, 4, idx, more, 4, 3, 0.2)):
        assert np.array_equal(a, b)
    # origins and fields take no names: their lanes are their own, and the two new words lie past them
    assert A._SPATIAL3_LANE > A._ELASTIC_LANE + 2 * A.elastic_nodes(1 << 16, 8) ** 2
    f = A.draw_elastic(2, 4, idx, (40, 40), 4.0, 8)
    assert np.array_equal(f, A.draw_elastic(2, 4, idx, (40, 40), 4.0, 8))
    # the in-plane angle and the zoom are draw_spatial's: at a vanishing out-of-plane range the block is its integers
    m2 = A.draw_spatial(2, 4, idx, "rotate", 30.0, 0.25)
    m3 = A.draw_spatial3(2, 4, idx, "rotate3d", 30.0, 0.0, 0.25)
    assert np.array_equal(m3, A.embed_mat3(m2))
    z2 = A.draw_spatial(2, 4, idx, "rotate,scale", 30.0, 0.25)
    z3 = A.draw_spatial3(2, 4, idx, "rotate3d,scale", 30.0, 0.0, 0.25)
    assert np.array_equal(z3, A.embed_mat3(z2))
    # scale3d zooms depth by the same z: entry 00 is rint(65536 / z), entry 11 at angle 0 too
    s3 = A.draw_spatial3(2, 4, idx, "scale3d", 30.0, 15.0, 0.25)
    assert np.array_equal(s3[:, 0], s3[:, 4]) and np.array_equal(s3[:, 4], A.draw_spatial(2, 4, idx, "scale")[:, 0])
    assert (s3[:, [1, 2, 3, 5, 6, 7]] == 0).all()


def test_draw_spatial3_is_the_documented_product():
    idx = np.arange(32)
    m = A.draw_spatial3(9, 1, idx, "rotate3d,scale3d", 30.0, 15.0, 0.25).reshape(-1, 3, 3).astype(np.float64) / ONE
    u = A._unit(A._hash(9, 1, idx, 2, first=A._SPATIAL_LANE))
    u3 = A._unit(A._hash(9, 1, idx, 2, first=A._SPATIAL3_LANE))
    for i in range(32):
        t0, t1, t2 = np.radians(30.0) * (2 * u[i, 0] - 1), np.radians(15.0) * (2 * u3[i, 0] - 1), \
            np.radians(15.0) * (2 * u3[i, 1] - 1)
        z = 1.25 ** (2 * u[i, 1] - 1)
        c, s = np.cos(t0), np.sin(t0)
        rd = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
        c, s = np.cos(t1), np.sin(t1)
        rh = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        c, s = np.cos(t2), np.sin(t2)
        rw = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        assert np.abs(m[i] - rd @ rh @ rw / z).max() <= 1.0 / ONE          # (rint, and the product's last bits)
        assert abs(np.linalg.det(m[i]) - z ** -3) < 1e-3
    assert (m[:, 0, 1] != 0).any() and (m[:, 0, 2] != 0).any() and (m[:, 1, 0] != 0).any()


# ------------------------------------------------------------------ warp3_torch
def test_embedded_matrices_equal_warp_torch_and_elastic_torch():
    """fd = 0: s0 * 1 + s1 * 0 is s0 exactly.  Stored (7, 40, 48), patch (4, 32, 32), all 16 codes."""
    x, y = _data((7, 40, 48), 3, 2, 16, seed=1)
    idx = np.arange(16)
    m2 = A.draw_spatial(4, 2, idx, "rotate,scale", 45.0, 0.5)
    org = A.draw_crop(4, 2, idx, (7, 40, 48), (4, 32, 32), "random")[0]
    code = np.arange(16, dtype=np.int32)
    ax, ay = A.warp_torch(x, y, org, (4, 32, 32), m2)
    bx, by = A.warp3_torch(x, y, org, (4, 32, 32), A.embed_mat3(m2))
    assert torch.equal(ax, bx) and torch.equal(ay, by) and (ax == 0).any() and (ax != 0).any()
    for u, v in zip(A.apply_torch(ax, ay, code), A.apply_torch(bx, by, code)):
        assert torch.equal(u, v)
    for S in (8, 32):
        f = A.draw_elastic(4, 2, idx, (32, 32), 4.0 if S == 32 else 1.0, S)
        ex, ey = A.elastic_torch(x, y, org, (4, 32, 32), m2, f, S)
        fx, fy = A.warp3_torch(x, y, org, (4, 32, 32), A.embed_mat3(m2), (f, S))
        assert torch.equal(ex, fx) and torch.equal(ey, fy) and not torch.equal(ex, ax)
    # a null origin on samples of the patch size, and tensors for arrays
    xs, ys = x[:, :4, :32, :32].contiguous(), y[:, :4, :32, :32].contiguous()
    ax, ay = A.warp_torch(xs, ys, None, (4, 32, 32), m2)
    bx, by = A.warp3_torch(xs, ys, None, (4, 32, 32), torch.from_numpy(A.embed_mat3(m2)))
    assert torch.equal(ax, bx) and torch.equal(ay, by)


def test_axis_permutations_are_exact():
    """Entries +-65536 that map depth onto h: a cubic patch strictly inside the volume comes out as
    the permuted / flipped crop, bit for bit."""
    x, y = _data((14, 15, 16), 2, 1, 3, seed=2)
    T = 8
    org = np.array([[2, 3, 4], [1, 1, 1], [5, 6, 7]])
    cx, cy = A.crop_torch(x, y, org, (T, T, T))
    # source (d, h, w) offset = M (output offset): out[d, h, w] = crop[h, d, w]
    swap = np.tile([0, ONE, 0, ONE, 0, 0, 0, 0, ONE], (3, 1))
    wx, wy = A.warp3_torch(x, y, org, (T, T, T), swap)
    assert torch.equal(wx, cx.permute(0, 2, 1, 3, 4)) and torch.equal(wy, cy.permute(0, 2, 1, 3, 4))
    # out[d, h, w] = crop[T-1-h, w, d]: depth from -h, h from w, w from d
    cyc = np.tile([0, -ONE, 0, 0, 0, ONE, ONE, 0, 0], (3, 1))
    wx, wy = A.warp3_torch(x, y, org, (T, T, T), cyc)
    assert torch.equal(wx, cx.permute(0, 3, 1, 2, 4).flip(2)) and torch.equal(wy, cy.permute(0, 3, 1, 2, 4).flip(2))
    # the depth flip
    fl = np.tile([-ONE, 0, 0, 0, ONE, 0, 0, 0, ONE], (3, 1))
    wx, wy = A.warp3_torch(x, y, org, (T, T, T), fl)
    assert torch.equal(wx, cx.flip(1)) and torch.equal(wy, cy.flip(1))


def test_half_voxel_depth_shift_is_the_mean_of_adjacent_slices():
    """Row 0 = (65536, 32768, 0) on a 3 x 3 x 3 patch: Qd = ((od + d) << 17) + 32768 u, and the rows
    u = -2, 0, +2 read depth od + d - 1/2 (fd = 65536 exactly), od + d and od + d + 1/2."""
    x, y = _data((6, 9, 9), 2, 1, 2, seed=3)
    org = np.array([[2, 3, 3], [1, 0, 5]])
    m = np.tile([ONE, ONE // 2, 0, 0, ONE, 0, 0, 0, ONE], (2, 1))
    wx, wy = A.warp3_torch(x, y, org, (3, 3, 3), m)
    cx = torch.stack([x[i, o[0] - 1:o[0] + 4, o[1]:o[1] + 3, o[2]:o[2] + 3] for i, o in enumerate(org)])   # slices od-1 .. od+3
    cy = torch.stack([y[i, o[0] - 1:o[0] + 4, o[1]:o[1] + 3, o[2]:o[2] + 3] for i, o in enumerate(org)])
    half = torch.tensor(0.5)
    for d in range(3):
        # row h = 0: source depth d - 1/2 (fd = 65536 exactly), row 1: d, row 2: d + 1/2
        assert torch.equal(wx[:, d, 0], cx[:, d, 0] * half + cx[:, d + 1, 0] * half)
        assert torch.equal(wx[:, d, 1], cx[:, d + 1, 1])
        assert torch.equal(wx[:, d, 2], cx[:, d + 1, 2] * half + cx[:, d + 2, 2] * half)
        # nearest: (Qd + 65536) >> 17 rounds the half up
        assert torch.equal(wy[:, d, 0], cy[:, d + 1, 0]) and torch.equal(wy[:, d, 2], cy[:, d + 2, 2])


def test_taps_outside_the_volume_are_zero_and_entries_are_clamped():
    x, y = _data((4, 8, 8), 1, 1, 1, seed=4)
    y = torch.ones_like(y)
    m = np.array([[2 * ONE, 0, 0, 0, ONE, 0, 0, 0, ONE]])                 # depth offset = 2 x output offset
    wx, wy = A.warp3_torch(x, y, None, (4, 8, 8), m)
    # t = -3, -1, 1, 3 -> source depth 1.5 + (-3, -1, 1, 3): -1.5, 0.5, 2.5, 4.5
    assert (wx[:, 0] == 0).all() and (wx[:, 3] == 0).all() and (wy[:, 0] == 0).all() and (wy[:, 3] == 0).all()
    half = torch.tensor(0.5)
    assert torch.equal(wx[:, 1], x[:, 0] * half + x[:, 1] * half) and (wy[:, 1] == 1).all()
    big = np.array([[1 << 20, -(1 << 20), 0, 5, 1 << 19, 0, 0, 0, -(1 << 30)]])
    a = A.warp3_torch(x, y, None, (4, 8, 8), big)
    b = A.warp3_torch(x, y, None, (4, 8, 8), np.clip(big, -(1 << 18), 1 << 18))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        A.warp3_torch(x[:, 0], y[:, 0], None, (1, 8, 8), m)               # 2D samples
    with pytest.raises(ValueError):
        A.warp3_torch(x, y, None, (4, 8, 8), m[:, :4])


# ------------------------------------------------------------------ config
def _cfg(**kw):
    return config.Config(**dict(dict(dims=3, img_size=16, depth=2, synthetic=True), **kw))


def test_parse_and_validate():
    assert config.parse_augment("rotate3d,scale3d") == ("rotate3d", "scale3d")
    assert config.SPATIAL_NAMES == ("rotate", "scale") and config.SPATIAL3_NAMES == ("rotate3d", "scale3d")
    config.validate(_cfg(augment="flip,rotate3d,scale3d,elastic,intensity", augment_elastic_cell=8, augment_elastic=1.0))
    config.validate(_cfg(augment="rotate3d,scale"))
    config.validate(_cfg(augment="rotate,scale3d", augment_rotate3d=180.0))
    for kw, word in ((dict(augment="rotate3d", dims=2), "rotate3d"), (dict(augment="flip,scale3d", dims=2), "scale3d"),
                     (dict(augment="rotate,rotate3d"), "rotate3d includes the in-plane rotation"),
                     (dict(augment="scale3d,scale"), "scale3d"),
                     (dict(augment_rotate3d=0.0), "--augment_rotate3d"), (dict(augment_rotate3d=180.5), "--augment_rotate3d"),
                     (dict(augment_rotate3d=-3.0), "--augment_rotate3d")):
        with pytest.raises(SystemExit) as e:
            config.validate(_cfg(**kw))
        assert word in str(e.value), (kw, str(e.value))
    assert config.parse_args(["--dims", "3", "--augment", "rotate3d", "--augment_rotate3d", "20"]).augment_rotate3d == 20.0
    assert config.Config().augment_rotate3d == 15.0


def test_make_aug_and_make_crop_aug_item_shapes():
    idx = np.array([1, 5, 6])
    for augment, width in (("flip,rotate3d", 9), ("scale3d", 9), ("rotate,scale3d", 9), ("rotate,scale", 4)):
        cfg = _cfg(augment=augment, in_channels=2, crop="random")
        out = A.make_aug(cfg, 3)(idx)
        assert len(out) == 3 and out[2].shape == (3, width) and out[2].dtype == np.int32
        out = A.make_crop_aug(cfg, 3, (20, 24, 28))(idx)
        assert len(out) == 4 and out[2].shape == (3, 3) and out[3].shape == (3, width)
    cfg = _cfg(augment="rotate3d,scale3d,elastic", augment_elastic_cell=8, augment_elastic=1.0, augment_rotate3d=20.0,
               crop="random")
    out = A.make_aug(cfg, 3)(idx)
    assert len(out) == 4 and out[2].shape == (3, 9) and out[3].shape == (3, 4, 4, 2)
    assert np.array_equal(out[2], A.draw_spatial3(cfg.seed, 3, idx, "rotate3d,scale3d", 30.0, 20.0, 0.25))
    out = A.make_crop_aug(cfg, 3, (20, 24, 28))(idx)
    assert len(out) == 5 and out[3].shape == (3, 9) and out[4].shape == (3, 4, 4, 2)
    assert A.has_spatial(("rotate3d",)) and A.has_spatial3(("scale3d",)) and not A.has_spatial3(("rotate", "scale"))


# ------------------------------------------------------------------ feeder and trainer
@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("elastic", [False, True])
def test_streamed_feeder_and_resident_batch_equal_warp3_torch(crop, elastic):
    from unet_distributed_amd.data.loader import DeviceFeeder, ResidentBatch
    rng = np.random.default_rng(4)
    S = (10, 20, 24) if crop else (8, 16, 16)
    patch = (8, 16, 16)
    x = rng.standard_normal((7,) + S + (2,)).astype(np.float32)
    y = (rng.random((7,) + S + (3,)) < 0.3).astype(np.float32)
    f = DeviceFeeder(x, y, 4, "cpu", patch=patch if crop else None, elastic_cell=8)
    assert not f.resident
    idx = np.array([6, 2, 5, 2])
    si = np.sort(idx)

    def aug(s):
        code, aff = A.draw(1, 2, s, "flip,rot90,intensity", 2, 3, 0.2)
        out = (code, aff) + ((A.draw_crop(1, 2, s, S, patch, "random")[0],) if crop else ())
        out += (A.draw_spatial3(1, 2, s, "rotate3d,scale3d", 30.0, 20.0, 0.5),)
        return out + ((A.draw_elastic(1, 2, s, (16, 16), 1.0, 8),) if elastic else ())

    drawn = aug(si)
    code, aff = drawn[:2]
    org = drawn[2] if crop else None
    mat = drawn[3 if crop else 2]
    field = drawn[-1] if elastic else None
    assert mat.shape == (4, 9)
    gx, gy = f.get(idx, aug=aug)
    wx, wy = A.warp3_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch, mat,
                           (field, 8) if elastic else None)
    assert (wx == 0).any() and (wx != 0).any()          # taps outside the volume and inside it
    wx, wy = A.apply_torch(wx, wy, code, aff)
    assert tuple(gx.shape) == (4, 8, 16, 16, 2) and torch.equal(gx, wx) and torch.equal(gy, wy)
    dev = (torch.from_numpy(code), torch.from_numpy(aff), torch.from_numpy(mat)) + (
        (torch.from_numpy(field),) if elastic else ())
    rb = ResidentBatch(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(si), dev,
                       (torch.from_numpy(org), patch) if crop else None, elastic_cell=8)
    tx, ty = rb.tensors()
    assert torch.equal(tx, wx) and torch.equal(ty, wy)


def test_cpu_trainer_feeds_the_torch_backend_warp3_torch(tmp_path, capsys):
    from unet_distributed_amd.runtime.trainer import Trainer
    log = tmp_path / "m.jsonl"
    cfg = config.Config(synthetic=True, synthetic_train=8, synthetic_test=4, batch_size=2, img_size=16, dims=3, depth=2,
                        synthetic_size=24, crop="random", in_channels=2, out_channels=1, device="cpu", backend="torch",
                        dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp_path), no_checkpoint=True, tensorboard=False,
                        export=False, resume=False, progress=False, steps=2, log_every=1000, log_jsonl=str(log),
                        augment="flip,rotate3d,scale3d,intensity", augment_rotate3d=20.0)
    config.validate(cfg)
    tr = Trainer(cfg)
    out = capsys.readouterr().out
    assert ("Training augmentation: flip, rotate3d, scale3d, intensity (amplitude 0.1) (rotate +-30 deg) "
            "(out of plane +-20 deg) (scale 0.8..1.25, depth too)\n") in out
    fed = {}
    inner = tr.backend.fwd_bwd

    def fwd_bwd(x, y, seed, **kw):
        fed[tr.flat.global_step] = (x.clone(), y.clone())
        return inner(x, y, seed, **kw)

    tr.backend.fwd_bwd = fwd_bwd
    res = tr.run()
    assert res["global_step"] == 2 and np.isfinite(res["train"]["loss"]) and sorted(fed) == [0, 1]
    epoch = tr.sampler.epoch_indices(0)
    for step in range(2):
        si = np.sort(epoch[step])
        code, aff = A.draw(cfg.seed, step, si, "flip,intensity", 2, 3, 0.1)
        mat = A.draw_spatial3(cfg.seed, step, si, "rotate3d,scale3d", 30.0, 20.0, 0.25)
        org = A.draw_crop(cfg.seed, step, si, (24, 24, 24), (16, 16, 16), "random")[0]
        wx, wy = A.warp3_torch(torch.from_numpy(tr.x_train[si]), torch.from_numpy(tr.y_train[si]), org, (16, 16, 16), mat)
        wx, wy = A.apply_torch(wx, wy, code, aff)
        assert torch.equal(fed[step][0], wx) and torch.equal(fed[step][1], wy)
    train = [r for r in (json.loads(line) for line in open(log)) if r["kind"] == "train"]
    assert train and train[-1]["augment"] == {"rotate_deg": [-30.0, 30.0], "rotate3d_deg": [-20.0, 20.0],
                                              "scale": [0.8, 1.25], "scale_depth": True}


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


@pytest.mark.parametrize("kind", ["gather_batch_warp3", "f32_gather_batch_warp3"])
def test_gather_batch_warp3_plan_time_validation(kind):
    C = _C()
    for dt in ((0, 1) if kind == "gather_batch_warp3" else (0,)):
        plan = C.Plan(dt)
        ptrs = [4096 * (i + 1) for i in range(10)]
        nofield = ptrs[:7] + [0] + ptrs[8:]
        # ints: B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K, s
        for ints in ([16, 20, 24, 28, 16, 16, 16, 4, 4, 2, 4], [2, 9, 40, 56, 5, 16, 16, 3, 32, 1, 5],
                     [8, 155, 240, 240, 128, 128, 128, 4, 4, 1, 5], [2, 1, 48, 48, 1, 32, 32, 4, 8, 3, 3]):
            for p in (ptrs, nofield, ptrs[:3] + [0, 0, ptrs[5], 0, 0] + ptrs[8:]):
                i = plan.add_generic(kind, p, ints, [], "gather")
                assert plan.check_dispatch(i, i + 1) == []
        # without a field s is not read
        i = plan.add_generic(kind, nofield, [2, 9, 40, 56, 5, 16, 16, 4, 4, 1, 0], [], "gather")
        assert plan.check_dispatch(i, i + 1) == []
        n0 = plan.size()
        bad = ([2, 8, 48, 48, 4, 32, 16, 4, 4, 1, 5],             # H != W
               [2, 8, 31, 48, 4, 32, 32, 4, 4, 1, 5], [2, 8, 48, 48, 16, 32, 32, 4, 4, 1, 5],     # patch > stored
               [2, 8, 48, 48, 4, 32, 32, 4, 4, 5, 5], [2, 8, 48, 48, 4, 32, 32, 8, 4, 1, 5],
               [2, 8, 48, 48, 0, 32, 32, 4, 4, 1, 5], [2, 1 << 20, 48, 48, 4, 32, 32, 4, 4, 1, 5],
               [1, 1 << 16, 8, 8, 1 << 16, 2, 2, 1, 1, 1, 5],     # D >= 2^16 (B D H W Cpad = 2^18: only this refuses)
               [2, 8, 48, 48, 4, 32, 32, 4, 4, 1, 2], [2, 8, 48, 48, 4, 32, 32, 4, 4, 1, 7])      # s, with a field
        for ints in bad:
            with pytest.raises(ValueError) as e:
                plan.add_generic(kind, ptrs, ints, [], "gather")
            assert "gather_batch_warp3" in str(e.value)
            with pytest.raises(ValueError):
                C.generic(kind, ptrs, ints, [], 0, dt)                   # (immediate style: nothing launched)
        with pytest.raises(ValueError) as e:
            plan.add_generic(kind, nofield, bad[7], [], "gather")
        assert "D >= 2^16" in str(e.value)
        i = plan.add_generic(kind, ptrs, [1, (1 << 16) - 1, 8, 8, (1 << 16) - 1, 2, 2, 1, 1, 1, 5], [], "gather")
        assert plan.check_dispatch(i, i + 1) == []
        n0 += 1
        good = [2, 8, 48, 48, 4, 32, 32, 4, 4, 1, 5]
        for missing in (0, 1, 2, 5, 8, 9):          # x_all, y_all, idx, mat, xb, tb
            with pytest.raises(ValueError):
                plan.add_generic(kind, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs[:9], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, good[:10], [], "")
        assert plan.size() == n0


def test_plan_check_knows_the_extents_of_the_warp3_ops():
    from unet_distributed_amd.runtime.plan_check import GATHER_OPS, _generic_rw, _generic_write_spans
    p = [4096 * (i + 1) for i in range(10)]
    ints = [8, 9, 40, 56, 5, 16, 16, 3, 4, 2, 3]
    px = 8 * 5 * 16 * 16                            # patch voxels: the stored size does not enter
    assert GATHER_OPS["gather_batch_warp3"].slots == ("origin", "code", "mat", "affine", "field")
    assert _generic_write_spans("gather_batch_warp3", p, ints) == [(p[8], px * 4 * 2), (p[9], px * 2 * 2)]
    assert _generic_write_spans("f32_gather_batch_warp3", p, ints) == [(p[8], px * 4 * 4), (p[9], px * 2 * 4)]
    assert _generic_rw("gather_batch_warp3", p, ints) == (p[:8], p[8:])
    assert _generic_rw("f32_gather_batch_warp3", p[:3] + [0, 0, p[5], 0, 0] + p[8:], ints) == (p[:3] + [p[5]], p[8:])


class _Flat:
    entries = ()


class _Engine:
    """What check_plan reads of an executor: named buffers and the target."""

    def __init__(self, bufs, target):
        self.bufs, self.target, self.flat = bufs, target, _Flat()


@pytest.mark.parametrize("kind,dtype", [("gather_batch_warp3", torch.bfloat16), ("f32_gather_batch_warp3", torch.float32)])
def test_check_plan_refuses_an_output_one_element_short(kind, dtype):
    from unet_distributed_amd.runtime.plan_check import RecordingPlan, check_plan
    B, S, T, cin, cpad, K = 2, (6, 12, 12), (4, 8, 8), 3, 4, 2
    vox = B * T[0] * T[1] * T[2]
    ins = {"x_all": torch.zeros((3,) + S + (cin,)), "y_all": torch.zeros((3,) + S + (K,)),
           "idx": torch.zeros(B, dtype=torch.int64), "origin": torch.zeros(B, 3, dtype=torch.int32),
           "code": torch.zeros(B, dtype=torch.int32), "mat": torch.zeros(B, 9, dtype=torch.int32),
           "affine": torch.zeros(B, cin, 2), "field": torch.zeros(B, 3, 3, 2, dtype=torch.int32)}
    ints = [B] + list(S) + list(T) + [cin, cpad, K, 3]
    for short_x, short_t in ((0, 0), (1, 0), (0, 1)):
        xb, tb = torch.zeros(vox * cpad - short_x, dtype=dtype), torch.zeros(vox * K - short_t, dtype=dtype)
        e = _Engine(dict(ins, x=xb), tb)
        plan = RecordingPlan(_C().Plan(0))
        plan.add_generic(kind, [int(t.data_ptr()) for t in ins.values()] + [int(xb.data_ptr()), int(tb.data_ptr())],
                         ints, [], "load")
        errs = check_plan(e, plan, False, extra_inputs=tuple(ins))
        if short_x or short_t:
            assert len(errs) == 1 and "past its end" in errs[0] and ("x+0" if short_x else "target+0") in errs[0], errs
        else:
            assert errs == []

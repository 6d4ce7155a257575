"""Rotate / scale augmentation off the GPU: the --augment rotate,scale flags, the counter-based
matrix draw (data/augment.py draw_spatial), warp_torch -- exact against crop_torch / apply_torch
where the matrix only moves pixels, against an independent float64 evaluation and
torch.nn.functional.grid_sample within the fp32 rounding bound elsewhere -- the streamed feeder,
the trainer on the ATen backend and plan-time validation of the gather_batch_warp ops."""
import json

import numpy as np
import pytest
import torch

from unet_distributed_amd import config
from unet_distributed_amd.data import augment as A

ONE = 65536


# ------------------------------------------------------------------ flags
def test_rotate_and_scale_flags_are_parsed_and_validated():
    cfg = config.Config()
    assert cfg.augment_rotate == 30.0 and cfg.augment_scale == 0.25
    assert "rotate" in config.AUGMENT_NAMES and "scale" in config.AUGMENT_NAMES
    assert config.parse_augment("flip,rot90,rotate,scale,intensity") == ("flip", "rot90", "rotate", "scale", "intensity")
    assert config.parse_augment("scale") == ("scale",)
    cfg = config.parse_args(["--augment", "rotate,scale", "--augment_rotate", "180", "--augment_scale", "1"])
    assert cfg.augment_rotate == 180.0 and cfg.augment_scale == 1.0
    with pytest.raises(SystemExit) as e:
        config.parse_augment("rotate,rotate")
    assert "'rotate'" in str(e.value) and "twice" in str(e.value)
    with pytest.raises(SystemExit) as e:
        config.parse_augment("flip,rot")
    assert "'rot'" in str(e.value) and "rotate" in str(e.value)       # names the item and the choices
    for flag, bad in (("--augment_rotate", ("0", "-5", "180.5", "nan")), ("--augment_scale", ("0", "-0.1", "1.5", "nan"))):
        for v in bad:
            with pytest.raises(SystemExit) as e:
                config.parse_args(["--augment", "rotate,scale", flag, v])
            assert flag in str(e.value), (flag, v)


# ------------------------------------------------------------------ draw
def test_draw_spatial_depends_only_on_seed_step_and_sample_index():
    idx = np.array([7, 0, 3, 3, 11, 2])
    m = A.draw_spatial(5, 9, idx, "rotate,scale", 30.0, 0.25)
    assert m.dtype == np.int32 and m.shape == (6, 4)
    perm = np.array([4, 2, 0, 5, 1, 3])
    assert np.array_equal(A.draw_spatial(5, 9, idx[perm], ("rotate", "scale"), 30.0, 0.25), m[perm])
    assert np.array_equal(np.concatenate([A.draw_spatial(5, 9, idx[:2], "rotate,scale"),
                                          A.draw_spatial(5, 9, idx[2:], "rotate,scale")]), m)
    assert np.array_equal(m[2], m[3])                                 # the repeated sample
    assert not np.array_equal(A.draw_spatial(5, 10, idx, "rotate,scale"), m)
    assert not np.array_equal(A.draw_spatial(6, 9, idx, "rotate,scale"), m)
    assert np.array_equal(m[:, 0], m[:, 3]) and np.array_equal(m[:, 1], -m[:, 2])
    # other names draw the identity
    assert np.array_equal(A.draw_spatial(5, 9, idx, "flip,intensity"), np.tile([ONE, 0, 0, ONE], (6, 1)))


def test_draw_and_draw_crop_do_not_change_with_rotate_and_scale():
    idx = np.arange(40)
    for dims in (2, 3):
        a = A.draw(3, 4, idx, "flip,rot90,intensity", 4, dims, 0.2)
        b = A.draw(3, 4, idx, "flip,rot90,intensity,rotate,scale", 4, dims, 0.2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(A.draw(3, 4, idx, "rotate,scale", 4, dims)[0], np.zeros(40, np.int32))
    o = A.draw_crop(3, 4, idx, (1, 48, 48), (1, 32, 32), "random")[0]

    class Cfg:
        seed, in_channels, dims, augment_intensity, img_size, crop = 3, 4, 2, 0.2, 32, "random"
        augment_rotate, augment_scale = 20.0, 0.5

    plain, spatial = Cfg(), Cfg()
    plain.augment, spatial.augment = "flip,rot90,intensity", "flip,rot90,intensity,rotate,scale"
    p, s = A.make_aug(plain, 4)(idx), A.make_aug(spatial, 4)(idx)
    assert len(p) == 2 and len(s) == 3
    assert np.array_equal(p[0], s[0]) and np.array_equal(p[1], s[1])
    assert np.array_equal(s[2], A.draw_spatial(3, 4, idx, "rotate,scale", 20.0, 0.5))
    p, s = A.make_crop_aug(plain, 4, (1, 48, 48))(idx), A.make_crop_aug(spatial, 4, (1, 48, 48))(idx)
    assert len(p) == 3 and len(s) == 4 and np.array_equal(p[2], o) and np.array_equal(s[2], o)
    assert np.array_equal(p[0], s[0]) and np.array_equal(p[1], s[1])
    assert np.array_equal(s[3], A.draw_spatial(3, 4, idx, "rotate,scale", 20.0, 0.5))


def test_draw_spatial_ranges():
    idx = np.arange(4000)
    r = A.draw_spatial(1, 2, idx, "rotate", 30.0, 0.25).astype(np.int64)
    # a rotation: a00^2 + a10^2 = 2^32 up to the two roundings, |error| <= 2 * 0.5 * 65536 * sqrt(2) + 0.5
    assert (np.abs(r[:, 0] ** 2 + r[:, 2] ** 2 - (1 << 32)) <= ONE * 2 ** 0.5 + 1).all()
    th = np.degrees(np.arctan2(r[:, 2], r[:, 0]))
    assert th.min() < -27 and th.max() > 27 and np.abs(th).max() <= 30 + 1e-3
    a = 0.25
    s = A.draw_spatial(1, 2, idx, "scale", 30.0, a).astype(np.int64)
    assert (s[:, 2] == 0).all() and (s[:, 1] == 0).all()
    lo, hi = int(np.rint(ONE / (1 + a))), int(np.rint(ONE * (1 + a)))
    assert (s[:, 0] >= lo).all() and (s[:, 0] <= hi).all()
    assert s[:, 0].min() < lo + 200 and s[:, 0].max() > hi - 300
    # log-uniform: the zoom is above 1 as often as below it
    assert abs(float((s[:, 0] < ONE).mean()) - 0.5) < 0.04


def test_mat_of_code():
    for c in range(8):
        m = A.mat_of_code(c)
        assert m.dtype == np.int32 and sorted(np.abs(m).tolist()) == [0, 0, ONE, ONE]
        assert (m[0] == 0) == bool(c & A.T)
    assert A.mat_of_code(0).tolist() == [ONE, 0, 0, ONE]
    with pytest.raises(ValueError):
        A.mat_of_code(8)


# ------------------------------------------------------------------ warp_torch: exact cases
def _data(shape, cin, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape + (cin,), generator=g)
    y = (torch.rand(shape + (K,), generator=g) > 0.6).float()
    return x, y


def test_warp_identity_is_the_crop():
    x, y = _data((6, 40, 48), 3, 2, 1)
    org = np.array([[0, 0, 0], [0, 8, 16], [0, 3, 5], [0, 8, 0], [0, 1, 16], [0, 7, 9]])    # maximum: taps past the edge
    eye = np.tile([ONE, 0, 0, ONE], (6, 1))
    wx, wy = A.warp_torch(x, y, org, (1, 32, 32), eye)
    cx, cy = A.crop_torch(x, y, org, (1, 32, 32))
    assert torch.equal(wx, cx) and torch.equal(wy, cy) and wx.is_contiguous()
    # no origin: the whole sample
    sx, sy = _data((3, 24, 24), 2, 1, 2)
    wx, wy = A.warp_torch(sx, sy, None, (24, 24), eye[:3])
    assert torch.equal(wx, sx) and torch.equal(wy, sy)
    # 3D: every slice through the same matrix, at the origin's depth
    x3, y3 = _data((2, 6, 20, 24), 2, 1, 3)
    o3 = np.array([[2, 1, 3], [0, 4, 8]])
    wx, wy = A.warp_torch(x3, y3, o3, (4, 16, 16), eye[:2])
    cx, cy = A.crop_torch(x3, y3, o3, (4, 16, 16))
    assert torch.equal(wx, cx) and torch.equal(wy, cy)


def test_warp_with_the_matrix_of_a_code_is_apply_torch():
    x, y = _data((4, 40, 48), 3, 2, 4)
    org = np.array([[0, 1, 1], [0, 7, 15], [0, 3, 8], [0, 4, 2]])     # strictly inside the stored image
    cx, cy = A.crop_torch(x, y, org, (1, 32, 32))
    for c in range(8):
        wx, wy = A.warp_torch(x, y, org, (1, 32, 32), np.tile(A.mat_of_code(c), (4, 1)))
        ax, ay = A.apply_torch(cx, cy, [c] * 4)
        assert torch.equal(wx, ax) and torch.equal(wy, ay), c


# ------------------------------------------------------------------ warp_torch: independent geometry
def _mats():
    def rot(deg, z):
        t = np.radians(deg)
        c, s = np.rint(ONE * np.cos(t) / z), np.rint(ONE * np.sin(t) / z)
        return [c, -s, s, c]
    return np.array([rot(45, 0.7), rot(10, 1.4), rot(-170, 1.0), rot(0, 1.0), rot(33.3, 0.9), rot(-80, 1.25)]
                    + A.draw_spatial(2, 3, np.arange(4), "rotate,scale", 180.0, 1.0).tolist(), dtype=np.int64)


def _float64_reference(x, y, org, patch, mat):
    """q = origin + (T - 1) / 2 + (m / 65536) (u, v) / 2 in float64 (exact: every term is a
    dyadic rational far below 2^53), floor / fraction, zero outside, bilinear in float64; the
    target at floor(q + 0.5)."""
    n, Hs, Ws = x.shape[0], x.shape[1], x.shape[2]
    H, W = patch
    xd, yd = x.double().numpy(), y.double().numpy()
    m = mat.astype(np.float64) / 65536.0
    u = (2.0 * np.arange(H) - (H - 1))[:, None]
    v = (2.0 * np.arange(W) - (W - 1))[None, :]
    xo, yo = np.zeros((n, H, W, x.shape[-1])), np.zeros((n, H, W, y.shape[-1]))
    qs = []
    for i in range(n):
        qh = org[i, 1] + (H - 1) / 2.0 + (m[i, 0] * u + m[i, 1] * v) / 2.0
        qw = org[i, 2] + (W - 1) / 2.0 + (m[i, 2] * u + m[i, 3] * v) / 2.0
        qs.append((qh, qw))
        ih, iw = np.floor(qh).astype(np.int64), np.floor(qw).astype(np.int64)
        fh, fw = (qh - ih)[..., None], (qw - iw)[..., None]

        def tap(src, r, c):
            ok = (r >= 0) & (r < Hs) & (c >= 0) & (c < Ws)
            return np.where(ok[..., None], src[np.clip(r, 0, Hs - 1), np.clip(c, 0, Ws - 1)], 0.0)

        xo[i] = ((tap(xd[i], ih, iw) * (1 - fw) + tap(xd[i], ih, iw + 1) * fw) * (1 - fh)
                 + (tap(xd[i], ih + 1, iw) * (1 - fw) + tap(xd[i], ih + 1, iw + 1) * fw) * fh)
        yo[i] = tap(yd[i], np.floor(qh + 0.5).astype(np.int64), np.floor(qw + 0.5).astype(np.int64))
    return xo, yo, qs


def test_warp_against_float64_and_grid_sample():
    """|warp_torch - float64| <= 2^-21 max|x|: at most nine fp32 roundings (four products, two
    sums, two products, one sum), each at most 2^-24 of a magnitude <= max|x| as the weights are
    convex -- 9 * 2^-24 < 2^-21.  The target is exact."""
    mat = _mats()
    n = len(mat)
    x, y = _data((n, 40, 48), 3, 2, 6)
    org = np.stack([np.zeros(n, int), np.arange(n) % 9, (3 * np.arange(n)) % 17], axis=1)
    H = W = 32
    wx, wy = A.warp_torch(x, y, org, (1, H, W), mat)
    rx, ry, qs = _float64_reference(x, y, org, (H, W), mat)
    bound = 2.0 ** -21 * float(x.abs().max())
    err = np.abs(wx.double().numpy() - rx).max()
    print("warp_torch vs float64: max err", err, "bound", bound)
    assert 0 < err <= bound
    assert np.array_equal(wy.numpy().astype(np.float64), ry)
    assert (wx[0] == 0).any() and (wy.numpy() != 0).any()             # 45 degrees at zoom 0.7 leaves the image
    # grid_sample, float64, align_corners=True (pixel = (g + 1) / 2 * (size - 1)), zeros outside
    Hs, Ws = 40, 48
    grid = torch.stack([torch.from_numpy(np.stack([2.0 * qw / (Ws - 1) - 1.0 for _, qw in qs])),
                        torch.from_numpy(np.stack([2.0 * qh / (Hs - 1) - 1.0 for qh, _ in qs]))], dim=-1)
    gs = torch.nn.functional.grid_sample(x.double().permute(0, 3, 1, 2), grid, mode="bilinear",
                                         padding_mode="zeros", align_corners=True).permute(0, 2, 3, 1)
    err = float((wx.double() - gs).abs().max())
    print("warp_torch vs grid_sample: max err", err, "bound", bound)
    assert 0 < err <= bound


def test_warp_clamps_the_matrix_and_the_origin():
    x, y = _data((3, 24, 28), 2, 1, 7)
    wild = np.array([[1 << 20, -(1 << 20), 1 << 19, -(1 << 30)], [-(1 << 20), 5, -7, 1 << 20], [ONE, 0, 0, ONE]])
    org = np.array([[0, -3, 100], [0, 9, -1], [5, 2 ** 31 - 1, -2 ** 31]])
    a = A.warp_torch(x, y, org, (1, 16, 16), wild)
    b = A.warp_torch(x, y, np.array([[0, 0, 12], [0, 8, 0], [0, 8, 0]]), (1, 16, 16), np.clip(wild, -(1 << 18), 1 << 18))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        A.warp_torch(x, y, None, (1, 32, 32), wild)                   # patch > stored
    with pytest.raises(ValueError):
        A.warp_torch(x, y, None, (1, 16, 16), wild[:2])


def test_zoom_one_half_without_crop_fills_with_zeros():
    x, y = _data((2, 16, 16), 3, 1, 8)
    y = torch.ones_like(y)
    m = np.tile([2 * ONE, 0, 0, 2 * ONE], (2, 1))                     # source offset = 2 x output offset
    wx, wy = A.warp_torch(x, y, None, (16, 16), m)
    for h, w in ((0, 0), (0, 15), (15, 0), (15, 15), (3, 8), (8, 12)):
        assert (wx[:, h, w] == 0).all() and (wy[:, h, w] == 0).all()
    # output (8, 8): u = v = 1, q = 7.5 + 1 = 8.5 -> the mean of source pixels 8..9 x 8..9 in the op's order
    half = torch.tensor(0.5)
    want = (x[:, 8, 8] * half + x[:, 8, 9] * half) * half + (x[:, 9, 8] * half + x[:, 9, 9] * half) * half
    assert torch.equal(wx[:, 8, 8], want) and (wy[:, 8, 8] == 1).all()
    # the image shrinks to the middle 8 x 8 (+ the half-covered ring); the target: q + 0.5 inside [0, 16)
    assert (wy[:, 4:12, 4:12] == 1).all() and (wy[:, :3] == 0).all() and (wy[:, :, 13:] == 0).all()


# ------------------------------------------------------------------ feeder and trainer
@pytest.mark.parametrize("crop", [False, True])
def test_streamed_feeder_and_resident_batch_equal_warp_torch(crop):
    from unet_distributed_amd.data.loader import DeviceFeeder, ResidentBatch
    rng = np.random.default_rng(4)
    S = (24, 28) if crop else (16, 16)
    patch = (1, 16, 16)
    x = rng.standard_normal((11,) + S + (4,)).astype(np.float32)
    y = (rng.random((11,) + S + (3,)) < 0.3).astype(np.float32)
    f = DeviceFeeder(x, y, 4, "cpu", patch=patch if crop else None)
    assert not f.resident
    idx = np.array([9, 2, 7, 2])
    si = np.sort(idx)

    def aug(s):
        code, aff = A.draw(1, 2, s, "flip,rot90,intensity", 4, 2, 0.2)
        mat = A.draw_spatial(1, 2, s, "rotate,scale", 45.0, 0.5)
        if crop:
            return code, aff, A.draw_crop(1, 2, s, (1,) + S, patch, "random")[0], mat
        return code, aff, mat

    drawn = aug(si)
    code, aff, mat = drawn[0], drawn[1], drawn[-1]
    org = drawn[2] if crop else None
    gx, gy = f.get(idx, aug=aug)
    wx, wy = A.warp_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch, mat)
    wx, wy = A.apply_torch(wx, wy, code, aff)
    assert tuple(gx.shape) == (4, 16, 16, 4) and torch.equal(gx, wx) and torch.equal(gy, wy)
    if crop:                        # the taps read the stored image outside the patch rectangle
        cx, _ = A.warp_torch(*A.crop_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch), None, patch, mat)
        assert not torch.equal(A.apply_torch(cx, wy, code, aff)[0], wx)
    rb = ResidentBatch(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(si),
                       (torch.from_numpy(code), torch.from_numpy(aff), torch.from_numpy(mat)),
                       (torch.from_numpy(org), patch) if crop else None)
    tx, ty = rb.tensors()
    assert torch.equal(tx, wx) and torch.equal(ty, wy) and rb.npix == 4 * 16 * 16 * 3
    # without matrices the feeder is what it was
    two = f.get(idx, aug=lambda s: aug(s)[:-1])
    base = A.crop_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch) if crop else \
        (torch.from_numpy(x[si]), torch.from_numpy(y[si]))
    bx, by = A.apply_torch(*base, code, aff)
    assert torch.equal(two[0], bx) and torch.equal(two[1], by)


def _trainer_cfg(tmp, **kw):
    base = dict(synthetic=True, synthetic_train=16, synthetic_test=8, batch_size=4, img_size=32, in_channels=4,
                out_channels=1, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False, steps=2,
                log_every=1000)
    return config.Config(**dict(base, **kw))


@pytest.mark.parametrize("crop", ["", "random"])
def test_cpu_trainer_feeds_the_torch_backend_warp_torch(tmp_path, capsys, crop):
    from unet_distributed_amd.runtime.trainer import Trainer
    log = tmp_path / "m.jsonl"
    tr = Trainer(_trainer_cfg(tmp_path, synthetic_size=48 if crop else 0, crop=crop, log_jsonl=str(log),
                              augment="flip,rot90,rotate,scale,intensity", augment_rotate=40.0, augment_scale=0.5))
    out = capsys.readouterr().out
    assert ("Training augmentation: flip, rot90, rotate, scale, intensity (amplitude 0.1) (rotate +-40 deg) "
            "(scale 0.6667..1.5)\n") in out
    fed = {}
    inner = tr.backend.fwd_bwd

    def fwd_bwd(x, y, seed, **kw):
        fed[tr.flat.global_step] = (x.clone(), y.clone())
        return inner(x, y, seed, **kw)

    tr.backend.fwd_bwd = fwd_bwd
    res = tr.run()
    assert res["global_step"] == 2 and np.isfinite(res["train"]["loss"]) and sorted(fed) == [0, 1]
    epoch = tr.sampler.epoch_indices(0)
    S = 48 if crop else 32
    for step in range(2):
        si = np.sort(epoch[step])
        code, aff = A.draw(tr.cfg.seed, step, si, "flip,rot90,intensity", 4, 2, 0.1)
        mat = A.draw_spatial(tr.cfg.seed, step, si, "rotate,scale", 40.0, 0.5)
        org = A.draw_crop(tr.cfg.seed, step, si, (S, S), (32, 32), "random")[0] if crop else None
        wx, wy = A.warp_torch(torch.from_numpy(tr.x_train[si]), torch.from_numpy(tr.y_train[si]), org, (32, 32), mat)
        wx, wy = A.apply_torch(wx, wy, code, aff)
        assert torch.equal(fed[step][0], wx) and torch.equal(fed[step][1], wy) and tuple(wx.shape) == (4, 32, 32, 4)
    recs = [json.loads(line) for line in open(log)]
    train = [r for r in recs if r["kind"] == "train"]
    assert train and train[-1]["augment"] == {"rotate_deg": [-40.0, 40.0], "scale": [1 / 1.5, 1.5]}
    assert all("augment" not in r for r in recs if r["kind"] != "train")     # a training-only transform


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


@pytest.mark.parametrize("kind", ["gather_batch_warp", "f32_gather_batch_warp"])
def test_gather_batch_warp_plan_time_validation(kind):
    C = _C()
    for dt in ((0, 1) if kind == "gather_batch_warp" else (0,)):
        plan = C.Plan(dt)
        ptrs = [4096 * (i + 1) for i in range(9)]
        # ints: B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K
        for ints in ([8, 1, 56, 40, 1, 32, 32, 4, 4, 3], [16, 20, 24, 28, 16, 16, 16, 4, 4, 2],
                     [2, 1, 16, 16, 1, 16, 16, 1, 4, 1], [2, 1, 40, 56, 1, 16, 16, 3, 32, 1],
                     [1024, 1, 240, 240, 1, 128, 128, 4, 4, 1], [8, 155, 240, 240, 128, 128, 128, 4, 4, 1]):
            i = plan.add_generic(kind, ptrs, ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
            # null origin, code and affine
            i = plan.add_generic(kind, ptrs[:3] + [0, 0, ptrs[5], 0] + ptrs[7:], ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
        n0 = plan.size()
        bad = ([2, 1, 48, 48, 1, 32, 16, 4, 4, 1],             # H != W
               [2, 1, 31, 48, 1, 32, 32, 4, 4, 1], [2, 1, 48, 31, 1, 32, 32, 4, 4, 1],      # patch > stored
               [2, 8, 48, 48, 16, 32, 32, 4, 4, 1],
               [2, 1, 48, 48, 1, 32, 32, 4, 4, 5], [2, 1, 48, 48, 1, 32, 32, 4, 4, 0],      # K outside 1..4
               [2, 1, 48, 48, 1, 32, 32, 8, 4, 1], [2, 1, 48, 48, 1, 32, 32, 4, 128, 1],    # Cin <= Cpad <= 64
               [2, 1, 48, 48, 0, 32, 32, 4, 4, 1], [0, 1, 48, 48, 1, 32, 32, 4, 4, 1],      # D, B >= 1
               [2, 1, 1 << 20, 48, 1, 32, 32, 4, 4, 1],                                      # stored side
               [1024, 1, 512, 512, 1, 512, 512, 8, 8, 1])                                    # >= 2^31
        for ints in bad:
            with pytest.raises(ValueError) as e:
                plan.add_generic(kind, ptrs, ints, [], "gather")
            assert "gather_batch_warp" in str(e.value)
            with pytest.raises(ValueError):
                C.generic(kind, ptrs, ints, [], 0, dt)                   # (immediate style: nothing launched)
        good = [2, 1, 48, 48, 1, 32, 32, 4, 4, 1]
        for missing in (0, 1, 2, 5, 7, 8):          # every pointer but origin, code and affine is required
            with pytest.raises(ValueError):
                plan.add_generic(kind, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs[:8], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, good[:9], [], "")
        assert plan.size() == n0


def test_plan_check_knows_the_extents_of_the_warp_ops():
    from unet_distributed_amd.runtime.plan_check import _generic_rw, _generic_write_spans
    p = [4096 * (i + 1) for i in range(9)]
    ints = [8, 5, 40, 56, 2, 16, 16, 3, 4, 2]
    px = 8 * 2 * 16 * 16                            # patch pixels: the stored size does not enter
    assert _generic_write_spans("gather_batch_warp", p, ints) == [(p[7], px * 4 * 2), (p[8], px * 2 * 2)]
    assert _generic_write_spans("f32_gather_batch_warp", p, ints) == [(p[7], px * 4 * 4), (p[8], px * 2 * 4)]
    assert _generic_rw("gather_batch_warp", p, ints) == (p[:7], p[7:])
    assert _generic_rw("f32_gather_batch_warp", p[:3] + [0, 0, p[5], 0] + p[7:], ints) == (p[:3] + [p[5]], p[7:])

"""Elastic augmentation off the GPU: the --augment elastic flags, the counter-based field draw
(data/augment.py draw_elastic), the integer quadratic B-spline displacement against a float64
spline, elastic_torch -- exact against warp_torch / crop_torch where the field is zero or
constant -- the streamed feeder, the trainer on the ATen backend and plan-time validation of the
gather_batch_elastic ops."""
import json

import numpy as np
import pytest
import torch

from unet_distributed_amd import config
from unet_distributed_amd.data import augment as A

ONE = 65536
PX = 1 << 17                    # one pixel in the field's unit


# ------------------------------------------------------------------ flags
def test_elastic_flags_are_parsed_and_validated():
    cfg = config.Config()
    assert cfg.augment_elastic == 4.0 and cfg.augment_elastic_cell == 32
    assert "elastic" in config.AUGMENT_NAMES and "elastic" not in config.SPATIAL_NAMES
    assert config.parse_augment("flip,rot90,rotate,scale,elastic,intensity")[4] == "elastic"
    cfg = config.parse_args(["--augment", "elastic", "--augment_elastic", "1.5", "--augment_elastic_cell", "16"])
    assert cfg.augment_elastic == 1.5 and cfg.augment_elastic_cell == 16
    config.parse_args(["--augment", "elastic", "--augment_elastic", "8", "--augment_elastic_cell", "64"])   # a == S / 8
    config.parse_args(["--augment", "elastic", "--augment_elastic", "1", "--augment_elastic_cell", "8"])
    # the three refusals name the value
    for argv, flag, val in ((["--augment_elastic_cell", "24"], "--augment_elastic_cell", "24"),
                            (["--augment_elastic_cell", "4", "--augment_elastic", "0.5"], "--augment_elastic_cell", "4"),
                            (["--augment_elastic_cell", "128"], "--augment_elastic_cell", "128"),
                            (["--augment_elastic", "0"], "--augment_elastic", "0"),
                            (["--augment_elastic", "-2"], "--augment_elastic", "-2"),
                            (["--augment_elastic", "nan"], "--augment_elastic", "nan"),
                            (["--augment_elastic", "4.5"], "--augment_elastic", "4.5"),                  # > 32 / 8
                            (["--augment_elastic", "2.5", "--augment_elastic_cell", "16"], "--augment_elastic", "2.5")):
        with pytest.raises(SystemExit) as e:
            config.parse_args(["--augment", "flip,elastic"] + argv)
        assert flag in str(e.value) and val in str(e.value), (argv, str(e.value))
    # the flags are validated only when elastic is named
    cfg = config.parse_args(["--augment", "flip", "--augment_elastic", "-1", "--augment_elastic_cell", "5"])
    assert cfg.augment_elastic == -1.0 and cfg.augment_elastic_cell == 5
    config.parse_args(["--augment_elastic", "100"])


# ------------------------------------------------------------------ draw
def test_draw_elastic_depends_only_on_seed_step_and_sample_index():
    idx = np.array([7, 0, 3, 3, 11, 2])
    f = A.draw_elastic(5, 9, idx, (40, 40), 2.0, 16)
    assert f.dtype == np.int32 and f.shape == (6, 5, 5, 2)            # N = (39 >> 4) + 3
    perm = np.array([4, 2, 0, 5, 1, 3])
    assert np.array_equal(A.draw_elastic(5, 9, idx[perm], (40, 40), 2.0, 16), f[perm])
    assert np.array_equal(np.concatenate([A.draw_elastic(5, 9, idx[:2], 40, 2.0, 16),
                                          A.draw_elastic(5, 9, idx[2:], 40, 2.0, 16)]), f)
    assert np.array_equal(f[2], f[3])                                  # the repeated sample
    assert not np.array_equal(A.draw_elastic(5, 10, idx, 40, 2.0, 16), f)
    assert not np.array_equal(A.draw_elastic(6, 9, idx, 40, 2.0, 16), f)
    # node counts: N = ((H - 1) >> s) + 3
    assert A.draw_elastic(1, 1, [0], 32, 1.0, 8).shape == (1, 6, 6, 2)
    assert A.draw_elastic(1, 1, [0], 32, 4.0, 64).shape == (1, 3, 3, 2)
    assert A.draw_elastic(1, 1, [0], 128).shape == (1, 6, 6, 2)       # the defaults: 4 px, cell 32
    assert A.draw_elastic(1, 1, [0], 33, 1.0, 32).shape == (1, 4, 4, 2)
    with pytest.raises(ValueError):
        A.draw_elastic(1, 1, [0], 32, 1.0, 24)


def test_draw_elastic_is_a_truncated_near_gaussian():
    a = 3.0
    f = A.draw_elastic(2, 3, np.arange(400), 128, a, 32).astype(np.float64) / PX        # 400 * 72 entries
    assert np.abs(f).max() <= 2 * a and np.abs(f).max() == 2 * a      # respects +-2a, and reaches it
    assert abs(f.mean()) < 0.05 * a
    # the standard deviation of the sum of four uniforms, scaled to unit variance and clipped at
    # +-2, from its density (four convolutions of a box on a fine grid); the sample's is within
    # 5 standard errors (sd / sqrt(2 n), n = 28800: 0.004)
    box = np.ones(512) / 512.0
    pdf = np.convolve(np.convolve(box, box), np.convolve(box, box))
    g = (np.arange(len(pdf)) / 512.0 - 2.0 + 1.5 / 512.0) / np.sqrt(4.0 / 12.0)
    sd = float(np.sqrt((pdf * np.clip(g, -2, 2) ** 2).sum()))
    assert 0.9 < sd < 1.0 and abs(f.std() / a - sd) < 0.02
    # the components and the nodes are independent draws
    flat = f.reshape(400, -1)
    c = np.corrcoef(flat[:, :8].T)
    assert np.abs(c - np.eye(8)).max() < 0.2
    # the definition, by hand, for one word
    h = A._hash(2, 3, np.array([5]), 2, first=A._ELASTIC_LANE)[0]
    t = [sum((int(w) >> (16 * k)) & 0xFFFF for k in range(4)) for w in h]
    want = [int(np.clip(np.rint(PX * a * (v - 131070) / np.sqrt((2 ** 32 - 1) / 3.0)), -2 * a * PX, 2 * a * PX))
            for v in t]
    assert A.draw_elastic(2, 3, [5], 128, a, 32)[0, 0, 0].tolist() == want


def test_draw_draw_crop_and_draw_spatial_do_not_change_with_elastic():
    idx = np.arange(40)
    for dims in (2, 3):
        a = A.draw(3, 4, idx, "flip,rot90,intensity", 4, dims, 0.2)
        b = A.draw(3, 4, idx, "flip,rot90,intensity,elastic", 4, dims, 0.2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(A.draw(3, 4, idx, "elastic", 4, dims)[0], np.zeros(40, np.int32))
    assert np.array_equal(A.draw_spatial(3, 4, idx, "rotate,scale,elastic", 20.0, 0.5),
                          A.draw_spatial(3, 4, idx, "rotate,scale", 20.0, 0.5))
    assert np.array_equal(A.draw_spatial(3, 4, idx, "elastic"), np.tile([ONE, 0, 0, ONE], (40, 1)))
    o = A.draw_crop(3, 4, idx, (1, 48, 48), (1, 32, 32), "random")[0]

    class Cfg:
        seed, in_channels, dims, augment_intensity, img_size, crop = 3, 4, 2, 0.2, 32, "random"
        augment_rotate, augment_scale, augment_elastic, augment_elastic_cell = 20.0, 0.5, 2.0, 16

    field = A.draw_elastic(3, 4, idx, (32, 32), 2.0, 16)
    mat = A.draw_spatial(3, 4, idx, "rotate,scale", 20.0, 0.5)
    for base, n_aug, n_crop in (("flip,rot90,intensity", 2, 3), ("flip,rot90,intensity,rotate,scale", 3, 4)):
        plain, el = Cfg(), Cfg()
        plain.augment, el.augment = base, base + ",elastic"
        p, s = A.make_aug(plain, 4)(idx), A.make_aug(el, 4)(idx)
        assert len(p) == n_aug and len(s) == 4                        # a tuple without elastic is today's tuple
        assert np.array_equal(p[0], s[0]) and np.array_equal(p[1], s[1]) and np.array_equal(s[3], field)
        assert (s[2] is None) if n_aug == 2 else (np.array_equal(s[2], mat) and np.array_equal(p[2], mat))
        p, s = A.make_crop_aug(plain, 4, (1, 48, 48))(idx), A.make_crop_aug(el, 4, (1, 48, 48))(idx)
        assert len(p) == n_crop and len(s) == 5 and np.array_equal(p[2], o) and np.array_equal(s[2], o)
        assert np.array_equal(p[0], s[0]) and np.array_equal(p[1], s[1]) and np.array_equal(s[4], field)
        assert (s[3] is None) if n_crop == 3 else (np.array_equal(s[3], mat) and np.array_equal(p[3], mat))
    only = Cfg()
    only.augment = "elastic"
    s = A.make_aug(only, 4)(idx)
    assert len(s) == 4 and s[1] is None and s[2] is None and not s[0].any() and np.array_equal(s[3], field)


# ------------------------------------------------------------------ the displacement
def _float64_spline(field, H, S):
    """The uniform quadratic B-spline through `field` [N][N][2] at the pixels 0..H-1 of both axes,
    in float64: weights [(1 - t)^2, -2 t^2 + 2 t + 1, t^2] / 2 at t = (p mod S) / S."""
    p = np.arange(H)
    c, t = p // S, (p % S) / float(S)
    w = np.stack([(1 - t) ** 2, -2 * t * t + 2 * t + 1, t * t]) / 2.0
    out = np.zeros((H, H, 2))
    for a in range(3):
        for b in range(3):
            out += (w[a][:, None] * w[b][None, :])[..., None] * field[(c + a)[:, None], (c + b)[None, :]].astype(np.float64)
    return out


@pytest.mark.parametrize("S,H", [(8, 40), (16, 40), (64, 100)])
def test_integer_displacement_is_within_one_unit_of_the_float64_spline(S, H):
    """d = floor(exact spline) (the weights sum to 4 S^4 = 2^(2 + 4 s) exactly), and the float64
    evaluation errs by far less than a unit on values below 2^23: |d - spline| < 1."""
    N = A.elastic_nodes(H, S)
    rng = np.random.default_rng(S)
    field = rng.integers(-(1 << 22), (1 << 22) + 1, size=(3, N, N, 2))
    field[1] = A.draw_elastic(1, 2, [9], H, S / 8.0, S)[0]
    field[2, ::2] = 1 << 22                                           # the extremes
    field[2, 1::2] = -(1 << 22)
    dh, dw = A.elastic_disp(field, (H, H), S)
    assert dh.dtype == torch.int64 and tuple(dh.shape) == (3, H, H)
    worst = 0.0
    for i in range(3):
        ref = _float64_spline(field[i], H, S)
        err = max(np.abs(dh[i].numpy() - ref[..., 0]).max(), np.abs(dw[i].numpy() - ref[..., 1]).max())
        worst = max(worst, err)
        assert err < 1.0, (S, i, err)
        assert (dh[i].numpy() <= ref[..., 0] + 1e-6).all()            # the shift is a floor
    print("integer displacement vs float64 spline, S", S, "max |err|", worst)
    assert worst > 0
    # a constant field is reproduced exactly, negative values included
    for k in (3 * PX, -5 * PX + 1, (1 << 22), -(1 << 22)):
        dh, dw = A.elastic_disp(np.full((1, N, N, 2), k), (H, H), S)
        assert (dh == k).all() and (dw == k).all()
    # the two components are independent: a field along h alone displaces along h alone
    f = np.zeros((1, N, N, 2), dtype=np.int64)
    f[..., 0] = field[0, ..., 0]
    dh0, dw0 = A.elastic_disp(f, (H, H), S)
    assert torch.equal(dh0[0], A.elastic_disp(field[:1], (H, H), S)[0][0]) and not dw0.any()


def test_displacement_gradient_is_at_most_one_half():
    """Nodes within +-2a and a <= S / 8: neighbouring pixels' displacements differ by at most
    half a pixel (plus the unit of the floor)."""
    for S in (8, 32):
        f = A.draw_elastic(4, 5, np.arange(8), 64, S / 8.0, S)
        dh, dw = A.elastic_disp(f, (64, 64), S)
        for d in (dh, dw):
            assert (d[:, 1:] - d[:, :-1]).abs().max() <= PX // 2 + 1
            assert (d[:, :, 1:] - d[:, :, :-1]).abs().max() <= PX // 2 + 1


# ------------------------------------------------------------------ elastic_torch: exact cases
def _data(shape, cin, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape + (cin,), generator=g)
    y = (torch.rand(shape + (K,), generator=g) > 0.6).float()
    return x, y


def _mats(n):
    def rot(deg, z):
        t = np.radians(deg)
        c, s = np.rint(ONE * np.cos(t) / z), np.rint(ONE * np.sin(t) / z)
        return [c, -s, s, c]
    rows = [rot(45, 0.7), rot(10, 1.4), rot(-170, 1.0), rot(0, 1.0), rot(33.3, 0.9), rot(-80, 1.25)]
    return np.array(rows[:n], dtype=np.int64)


def test_zero_field_is_warp_torch():
    x, y = _data((6, 40, 48), 3, 2, 1)
    org = np.array([[0, 0, 0], [0, 8, 16], [0, 3, 5], [0, 8, 0], [0, 1, 16], [0, 7, 9]])
    mat = _mats(6)
    for S in (8, 16, 32, 64):
        zero = np.zeros((6, A.elastic_nodes(32, S), A.elastic_nodes(32, S), 2), dtype=np.int32)
        ex, ey = A.elastic_torch(x, y, org, (1, 32, 32), mat, zero, S)
        wx, wy = A.warp_torch(x, y, org, (1, 32, 32), mat)
        assert torch.equal(ex, wx) and torch.equal(ey, wy) and ex.is_contiguous()
        # no matrix: the identity, which is the crop
        ex, ey = A.elastic_torch(x, y, org, (1, 32, 32), None, zero, S)
        cx, cy = A.crop_torch(x, y, org, (1, 32, 32))
        assert torch.equal(ex, cx) and torch.equal(ey, cy)
    # 3D: every slice through the same field; no origin: the whole sample
    x3, y3 = _data((2, 6, 20, 24), 2, 1, 3)
    o3 = np.array([[2, 1, 3], [0, 4, 8]])
    f3 = A.draw_elastic(1, 2, [0, 1], 16, 1.0, 8)
    ex, ey = A.elastic_torch(x3, y3, o3, (4, 16, 16), None, f3, 8)
    flat = o3 * np.array([0, 1, 1])
    for d in range(4):
        xs, ys = torch.stack([x3[0, 2 + d], x3[1, d]]), torch.stack([y3[0, 2 + d], y3[1, d]])
        sx, sy = A.elastic_torch(xs, ys, flat, (1, 16, 16), None, f3, 8)
        assert torch.equal(ex[:, d], sx) and torch.equal(ey[:, d], sy)
    wx, wy = A.elastic_torch(x3, y3, None, (6, 20, 20), None, A.draw_elastic(1, 2, [0, 1], 20, 1.0, 8), 8)
    assert tuple(wx.shape) == (2, 6, 20, 20, 2) and tuple(wy.shape) == (2, 6, 20, 20, 1)


def test_constant_field_is_the_crop_at_the_shifted_origin():
    x, y = _data((4, 40, 48), 3, 2, 4)
    org = np.array([[0, 3, 4], [0, 5, 9], [0, 2, 12], [0, 4, 2]])
    N = A.elastic_nodes(32, 16)
    for kh, kw in ((2, 3), (-2, 1), (0, -1), (3, -2)):                # the patch stays inside the image
        field = np.zeros((4, N, N, 2), dtype=np.int32)
        field[..., 0], field[..., 1] = kh * PX, kw * PX
        ex, ey = A.elastic_torch(x, y, org, (1, 32, 32), None, field, 16)
        cx, cy = A.crop_torch(x, y, org + [0, kh, kw], (1, 32, 32))
        assert torch.equal(ex, cx) and torch.equal(ey, cy), (kh, kw)
    # half a pixel along w: the mean of two neighbours in the op's order; the target rounds up
    field = np.zeros((4, N, N, 2), dtype=np.int32)
    field[..., 1] = PX // 2
    ex, ey = A.elastic_torch(x, y, org, (1, 32, 32), None, field, 16)
    cx0, cy0 = A.crop_torch(x, y, org, (1, 32, 32))
    cx1, cy1 = A.crop_torch(x, y, org + [0, 0, 1], (1, 32, 32))
    half = torch.tensor(0.5)                                           # (the row weights are 1 and 0)
    assert torch.equal(ex, cx0 * half + cx1 * half) and torch.equal(ey, cy1)


def test_the_displacement_is_indexed_before_the_code():
    """The whole transform is apply_torch(elastic_torch(...), code): a field that displaces one
    corner of the patch alone moves the pixels that corner lands on after the flips and the swap."""
    x, y = _data((8, 48, 48), 2, 1, 5)
    org = np.tile([0, 8, 8], (8, 1))
    N = A.elastic_nodes(32, 8)
    field = np.zeros((8, N, N, 2), dtype=np.int32)
    field[:, 0, 0, 0] = 3 * PX                                         # the node that reaches patch pixels h', w' < 8 only
    ex, ey = A.elastic_torch(x, y, org, (1, 32, 32), None, field, 8)
    cx, cy = A.crop_torch(x, y, org, (1, 32, 32))
    moved = (ex != cx).any(dim=-1)
    assert moved[:, :8, :8].any() and not moved[:, 8:].any() and not moved[:, :, 8:].any()
    code = np.arange(8)
    ax, _ = A.apply_torch(ex, ey, code)
    bx, _ = A.apply_torch(cx, cy, code)
    mv = (ax != bx).any(dim=-1)
    for c in range(8):
        hs = slice(24, 32) if c & (A.FW if c & A.T else A.FH) else slice(0, 8)
        ws = slice(24, 32) if c & (A.FH if c & A.T else A.FW) else slice(0, 8)
        inside = torch.zeros(32, 32, dtype=torch.bool)
        inside[hs, ws] = True
        assert mv[c][inside].any() and not mv[c][~inside].any(), c


def test_field_entries_beyond_the_clamp_read_as_the_clamped_values():
    x, y = _data((3, 40, 48), 2, 1, 7)
    N = A.elastic_nodes(32, 32)
    rng = np.random.default_rng(3)
    wild = rng.integers(-(1 << 31), 1 << 31, size=(3, N, N, 2)).astype(np.int64)
    wild[0, 0, 0] = [(1 << 22) + 1, -(1 << 22) - 1]
    wild[1] = (1 << 31) - 1
    org = np.array([[0, 4, 8], [0, 0, 0], [0, 8, 16]])
    a = A.elastic_torch(x, y, org, (1, 32, 32), _mats(3), wild.astype(np.int32), 32)
    b = A.elastic_torch(x, y, org, (1, 32, 32), _mats(3), np.clip(wild, -(1 << 22), 1 << 22), 32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert A.FIELD_MAX == 1 << 22
    # sample 1 is displaced by 32 pixels along both axes: it reads the stored image there, zero outside
    c = A.elastic_torch(x[1:2], y[1:2], None, (1, 8, 8), None, np.full((1, 3, 3, 2), 1 << 30, dtype=np.int32), 32)
    assert torch.equal(c[0][0], x[1, 32:40, 32:40]) and torch.equal(c[1][0], y[1, 32:40, 32:40])
    with pytest.raises(ValueError):
        A.elastic_torch(x, y, org, (1, 32, 32), None, wild[:, :2].astype(np.int32), 32)     # the field's shape
    with pytest.raises(ValueError):
        A.elastic_torch(x, y, org, (1, 32, 32), None, wild[:2].astype(np.int32), 32)
    with pytest.raises(ValueError):
        A.elastic_torch(x, y, org, (1, 64, 64), None, wild.astype(np.int32), 32)            # patch > stored


# ------------------------------------------------------------------ feeder and trainer
@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("spatial", [False, True])
def test_streamed_feeder_and_resident_batch_equal_elastic_torch(crop, spatial):
    from unet_distributed_amd.data.loader import DeviceFeeder, ResidentBatch
    rng = np.random.default_rng(4)
    S = (24, 28) if crop else (16, 16)
    patch = (1, 16, 16)
    x = rng.standard_normal((11,) + S + (4,)).astype(np.float32)
    y = (rng.random((11,) + S + (3,)) < 0.3).astype(np.float32)
    f = DeviceFeeder(x, y, 4, "cpu", patch=patch if crop else None, elastic_cell=8)
    assert not f.resident
    idx = np.array([9, 2, 7, 2])
    si = np.sort(idx)

    def aug(s):
        code, aff = A.draw(1, 2, s, "flip,rot90,intensity", 4, 2, 0.2)
        mat = A.draw_spatial(1, 2, s, "rotate,scale", 45.0, 0.5) if spatial else None
        field = A.draw_elastic(1, 2, s, 16, 1.0, 8)
        if crop:
            return code, aff, A.draw_crop(1, 2, s, (1,) + S, patch, "random")[0], mat, field
        return code, aff, mat, field

    drawn = aug(si)
    code, aff, mat, field = drawn[0], drawn[1], drawn[-2], drawn[-1]
    org = drawn[2] if crop else None
    gx, gy = f.get(idx, aug=aug)
    wx, wy = A.elastic_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch, mat, field, 8)
    wx, wy = A.apply_torch(wx, wy, code, aff)
    assert tuple(gx.shape) == (4, 16, 16, 4) and torch.equal(gx, wx) and torch.equal(gy, wy)
    # the field matters
    zx, _ = A.elastic_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch, mat, np.zeros_like(field), 8)
    assert not torch.equal(A.apply_torch(zx, wy, code, aff)[0], wx)
    rb = ResidentBatch(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(si),
                       (torch.from_numpy(code), torch.from_numpy(aff), torch.from_numpy(mat) if spatial else None,
                        torch.from_numpy(field)), (torch.from_numpy(org), patch) if crop else None, elastic_cell=8)
    tx, ty = rb.tensors()
    assert torch.equal(tx, wx) and torch.equal(ty, wy) and rb.npix == 4 * 16 * 16 * 3
    # without the field the feeder is what it was
    def plain(s):
        d = aug(s)
        return (d[:3] if crop else d[:2]) + ((d[-2],) if spatial else ())

    two = f.get(idx, aug=plain)
    if spatial:
        bx, by = A.warp_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch, mat)
    else:
        bx, by = A.crop_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), org, patch) if crop else \
            (torch.from_numpy(x[si]), torch.from_numpy(y[si]))
    bx, by = A.apply_torch(bx, by, code, aff)
    assert torch.equal(two[0], bx) and torch.equal(two[1], by)


def _trainer_cfg(tmp, **kw):
    base = dict(synthetic=True, synthetic_train=16, synthetic_test=8, batch_size=4, img_size=32, in_channels=4,
                out_channels=1, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False, steps=2,
                log_every=1000)
    return config.Config(**dict(base, **kw))


@pytest.mark.parametrize("crop,augment", [("", "flip,rot90,elastic,intensity"),
                                          ("random", "flip,rot90,rotate,scale,elastic,intensity")])
def test_cpu_trainer_feeds_the_torch_backend_elastic_torch(tmp_path, capsys, crop, augment):
    from unet_distributed_amd.runtime.trainer import Trainer
    log = tmp_path / "m.jsonl"
    spatial = "rotate" in augment
    tr = Trainer(_trainer_cfg(tmp_path, synthetic_size=48 if crop else 0, crop=crop, log_jsonl=str(log),
                              augment=augment, augment_rotate=40.0, augment_scale=0.5, augment_elastic=2.0,
                              augment_elastic_cell=16))
    out = capsys.readouterr().out
    if spatial:
        assert ("Training augmentation: flip, rot90, rotate, scale, elastic, intensity (amplitude 0.1) "
                "(rotate +-40 deg) (scale 0.6667..1.5) (elastic sigma 2 px, cell 16)\n") in out
    else:
        assert "Training augmentation: flip, rot90, elastic, intensity (amplitude 0.1) (elastic sigma 2 px, cell 16)\n" in out
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
        mat = A.draw_spatial(tr.cfg.seed, step, si, "rotate,scale", 40.0, 0.5) if spatial else None
        field = A.draw_elastic(tr.cfg.seed, step, si, 32, 2.0, 16)
        org = A.draw_crop(tr.cfg.seed, step, si, (S, S), (32, 32), "random")[0] if crop else None
        wx, wy = A.elastic_torch(torch.from_numpy(tr.x_train[si]), torch.from_numpy(tr.y_train[si]), org, (32, 32),
                                 mat, field, 16)
        wx, wy = A.apply_torch(wx, wy, code, aff)
        assert torch.equal(fed[step][0], wx) and torch.equal(fed[step][1], wy) and tuple(wx.shape) == (4, 32, 32, 4)
    recs = [json.loads(line) for line in open(log)]
    train = [r for r in recs if r["kind"] == "train"]
    want = {"elastic": {"sigma_px": 2.0, "cell": 16}}
    if spatial:
        want.update({"rotate_deg": [-40.0, 40.0], "scale": [1 / 1.5, 1.5]})
    assert train and train[-1]["augment"] == want
    assert all("augment" not in r for r in recs if r["kind"] != "train")


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


@pytest.mark.parametrize("kind", ["gather_batch_elastic", "f32_gather_batch_elastic"])
def test_gather_batch_elastic_plan_time_validation(kind):
    C = _C()
    for dt in ((0, 1) if kind == "gather_batch_elastic" else (0,)):
        plan = C.Plan(dt)
        ptrs = [4096 * (i + 1) for i in range(10)]
        # ints: B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K, s
        for ints in ([8, 1, 56, 40, 1, 32, 32, 4, 4, 3, 3], [16, 20, 24, 28, 16, 16, 16, 4, 4, 2, 4],
                     [2, 1, 16, 16, 1, 16, 16, 1, 4, 1, 6], [2, 1, 40, 56, 1, 16, 16, 3, 32, 1, 5],
                     [1024, 1, 240, 240, 1, 128, 128, 4, 4, 1, 5], [8, 155, 240, 240, 128, 128, 128, 4, 4, 1, 5]):
            i = plan.add_generic(kind, ptrs, ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
            # null origin, code, matrix and affine
            i = plan.add_generic(kind, ptrs[:3] + [0, 0, 0, 0] + ptrs[7:], ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
        n0 = plan.size()
        bad = ([2, 1, 48, 48, 1, 32, 16, 4, 4, 1, 5],             # H != W
               [2, 1, 31, 48, 1, 32, 32, 4, 4, 1, 5], [2, 1, 48, 31, 1, 32, 32, 4, 4, 1, 5],      # patch > stored
               [2, 8, 48, 48, 16, 32, 32, 4, 4, 1, 5],
               [2, 1, 48, 48, 1, 32, 32, 4, 4, 5, 5], [2, 1, 48, 48, 1, 32, 32, 4, 4, 0, 5],      # K outside 1..4
               [2, 1, 48, 48, 1, 32, 32, 8, 4, 1, 5], [2, 1, 48, 48, 1, 32, 32, 4, 128, 1, 5],    # Cin <= Cpad <= 64
               [2, 1, 48, 48, 0, 32, 32, 4, 4, 1, 5], [0, 1, 48, 48, 1, 32, 32, 4, 4, 1, 5],      # D, B >= 1
               [2, 1, 1 << 20, 48, 1, 32, 32, 4, 4, 1, 5],                                         # stored side
               [1024, 1, 512, 512, 1, 512, 512, 8, 8, 1, 5],                                       # >= 2^31
               [2, 1, 48, 48, 1, 32, 32, 4, 4, 1, 2], [2, 1, 48, 48, 1, 32, 32, 4, 4, 1, 7],      # 3 <= s <= 6
               [2, 1, 48, 48, 1, 32, 32, 4, 4, 1, 0], [2, 1, 48, 48, 1, 32, 32, 4, 4, 1, -1],
               [2, 1, 48, 48, 1, 32, 32, 4, 4, 1, 32])                                             # (the side, not its log2)
        for ints in bad:
            with pytest.raises(ValueError) as e:
                plan.add_generic(kind, ptrs, ints, [], "gather")
            assert "gather_batch_elastic" in str(e.value)
            with pytest.raises(ValueError):
                C.generic(kind, ptrs, ints, [], 0, dt)                   # (immediate style: nothing launched)
        good = [2, 1, 48, 48, 1, 32, 32, 4, 4, 1, 5]
        for missing in (0, 1, 2, 7, 8, 9):          # every pointer but origin, code, matrix and affine is required
            with pytest.raises(ValueError):
                plan.add_generic(kind, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs[:9], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, good[:10], [], "")
        assert plan.size() == n0


def test_plan_check_knows_the_extents_of_the_elastic_ops():
    from unet_distributed_amd.runtime.plan_check import _generic_rw, _generic_write_spans
    p = [4096 * (i + 1) for i in range(10)]
    ints = [8, 5, 40, 56, 2, 16, 16, 3, 4, 2, 3]
    px = 8 * 2 * 16 * 16                            # patch pixels: the stored size does not enter
    assert _generic_write_spans("gather_batch_elastic", p, ints) == [(p[8], px * 4 * 2), (p[9], px * 2 * 2)]
    assert _generic_write_spans("f32_gather_batch_elastic", p, ints) == [(p[8], px * 4 * 4), (p[9], px * 2 * 4)]
    assert _generic_rw("gather_batch_elastic", p, ints) == (p[:8], p[8:])
    assert _generic_rw("f32_gather_batch_elastic", p[:3] + [0, 0, 0, 0] + p[7:], ints) == (p[:3] + [p[7]], p[8:])
    # the warp's entries are what they were
    assert _generic_write_spans("gather_batch_warp", p[:9], ints[:10]) == [(p[7], px * 4 * 2), (p[8], px * 2 * 2)]

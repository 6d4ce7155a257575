"""Sliding-window inference on the CPU (ops/sliding.py: geometry and the torch oracle the HIP
kernels of csrc/kernels/sliding.h are held to), the static validation of the executors'
`sw_plan`, the plan-time refusals of the three generic ops and the command line.

Rounding of a pointwise predictor.  A pixel covered by n tiles gets
acc = ((w_1 p (1 + d_1)) + w_2 p (1 + d_2)) (1 + a_2) + ..., every |d|, |a| <= 2^-24: n products,
n - 1 additions of positive terms, so acc = p W (1 + e) with |e| <= (2 n - 1) 2^-24 to first order,
W the exact weight sum; wsum = W (1 + e') with |e'| <= (n - 1) 2^-24; the division adds 2^-24.
 * n = 1: result = fl(fl(w p) / w), |error| <= 2 * 2^-24 p < 2 ulp(p) -- the 2 ulp of the
   specification, for any weight map.
 * constant weights with n in {1, 2, 4}: the products and wsum are exact, p + p is exact, the two
   further additions round once each: |error| <= 2 * 2^-24 p again, the division by 2 or 4 is exact.
 * in general the bound is (3 n - 1) 2^-24 p, which for the Gaussian map at overlap 0.5 in 2D
   (n up to 6 with a clamped last tile) is far past 2 ulp: 4 ulp are reached in practice.  Those
   cases are held to the derived per-pixel bound instead.
"""
import numpy as np
import pytest
import torch

from unet_distributed_amd.ops import sliding

EPS = 2.0 ** -24

# (image dims, tile, stride) of every geometry the GPU tests use (tests/test_gpu_sliding.py)
GPU_GEOMETRIES = [((1, 40, 56), (1, 32, 32), s) for s in ((1, 16, 16), (1, 32, 32), (1, 8, 8))] + \
                 [((1, 24, 72), (1, 32, 32), s) for s in ((1, 16, 16), (1, 32, 32), (1, 8, 8))] + \
                 [((1, 32, 32), (1, 32, 32), (1, 16, 16)), ((1, 44, 52), (1, 32, 32), (1, 16, 16)),
                  ((40, 32, 48), (32, 32, 32), (16, 16, 16))]


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("dims,T,stride", GPU_GEOMETRIES)
def test_origins_cover_clamp_and_increase(dims, T, stride):
    for L, t, s in zip(dims, T, stride):
        o = sliding.tile_origins(L, t, s)
        if L <= t:
            assert o == [0]
            continue
        assert o[0] == 0 and o[-1] == L - t, "the last tile ends at the edge"
        assert all(b > a for a, b in zip(o, o[1:])), "strictly increasing"
        assert all(b - a <= s for a, b in zip(o, o[1:])), "no gap wider than the stride"
        assert o[:-1] == [i * s for i in range(len(o) - 1)] and len(o) == -(-(L - t) // s) + 1
        covered = np.zeros(L, bool)
        for a in o:
            assert 0 <= a and a + t <= L
            covered[a:a + t] = True
        assert covered.all()


def test_origins_of_a_brats_volume():
    T = sliding.tile_shape(128, 3)
    stride = sliding.strides(T, 0.5)
    assert T == (128, 128, 128) and stride == (64, 64, 64)
    assert sliding.grid_origins((155, 240, 240), T, stride) == [[0, 27], [0, 64, 112], [0, 64, 112]]
    assert sliding.tiles_per_image((155, 240, 240), T, stride) == 18
    tl = sliding.tile_list((155, 240, 240), T, stride)
    assert tl[0] == (0, 0, 0) and tl[1] == (0, 0, 64) and tl[3] == (0, 64, 0) and tl[-1] == (27, 112, 112)
    # 2D: the slice axis has tile 1 and stride 1
    assert sliding.tile_shape(128, 2) == (1, 128, 128) and sliding.strides((1, 128, 128), 0.5) == (1, 64, 64)
    assert sliding.strides((1, 32, 32), 0.75) == (1, 8, 8) and sliding.strides((1, 32, 32), 0.0) == (1, 32, 32)
    assert sliding.strides((1, 30, 30), 0.3) == (1, 21, 21)


def test_errors_name_the_bad_value():
    for bad in (-0.1, 0.8, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 0\.75\].*%s" % ("nan" if bad != bad else repr(bad))):
            sliding.strides((1, 32, 32), bad)
    with pytest.raises(ValueError, match="constant \\| gaussian.*'cosine'"):
        sliding.weight_map((1, 8, 8), "cosine")
    with pytest.raises(ValueError, match="'cosine'"):
        sliding.sliding_predict_torch(lambda t: t, torch.zeros(1, 8, 8, 1), (1, 8, 8), 2, 0.5, "cosine")
    with pytest.raises(ValueError, match="0.9"):
        sliding.sliding_predict_torch(lambda t: t, torch.zeros(1, 8, 8, 1), (1, 8, 8), 2, 0.9, "constant")
    with pytest.raises(ValueError, match="shape"):
        sliding.sliding_predict_torch(lambda t: t, torch.zeros(8, 8, 1), (1, 8, 8), 2, 0.5, "constant")


def test_weight_maps():
    w = sliding.weight_map((1, 32, 32), "gaussian")
    assert w.dtype == torch.float32 and tuple(w.shape) == (1, 32, 32)
    i = np.arange(32, dtype=np.float64)
    g = np.exp(-0.5 * ((i - 15.5) / 4.0) ** 2)
    assert np.array_equal(w[0].numpy(), (g[:, None] * g[None, :]).astype(np.float32))
    assert torch.equal(w, w.flip(1)) and torch.equal(w, w.flip(2)) and torch.equal(w[0], w[0].t())
    assert torch.equal(sliding.weight_map((2, 3, 4), "constant"), torch.ones(2, 3, 4))
    # 128^3: the smallest weight is a normal fp32 number (no clamp needed); per axis, not the 2M-element product
    g = sliding.weight_map((1, 1, 128), "gaussian").double().min()
    assert 5.0e-11 < float(g) ** 3 < 6.0e-11 and float(g) ** 3 > float(np.finfo(np.float32).tiny)


@pytest.mark.parametrize("dims,T,stride", GPU_GEOMETRIES)
@pytest.mark.parametrize("blend", sliding.BLENDS)
def test_wsum_is_positive_everywhere(dims, T, stride, blend):
    ws = sliding.weight_sum(dims, T, stride, blend)
    assert tuple(ws.shape) == dims and ws.dtype == torch.float32 and bool((ws > 0).all())
    if blend == "constant":                 # the number of covering tiles
        cnt = torch.zeros(dims)
        for o in sliding.tile_list(dims, T, stride):
            cnt[o[0]:o[0] + T[0], o[1]:o[1] + T[1], o[2]:o[2] + T[2]] += 1
        assert torch.equal(ws, cnt)


# ------------------------------------------------------------------ oracle properties
def _tiles(dims, T, stride, N, K, seed, ones=False):
    total = N * sliding.tiles_per_image(dims, T, stride)
    g = torch.Generator().manual_seed(seed)
    return torch.ones((total,) + T + (K,)) if ones else torch.rand((total,) + T + (K,), generator=g)


@pytest.mark.parametrize("dims,T,stride", GPU_GEOMETRIES)
@pytest.mark.parametrize("blend", sliding.BLENDS)
def test_blend_range_and_ones(dims, T, stride, blend):
    N, K = 2, 3
    ws = sliding.weight_sum(dims, T, stride, blend)
    p = _tiles(dims, T, stride, N, K, 7)
    p[0], p[-1, ..., 0] = 0.0, 1.0
    acc = sliding.blend_tiles_torch(p, torch.zeros((N,) + dims + (K,)), T, stride, blend)
    assert bool((acc >= 0).all()) and bool((acc <= ws[None, ..., None]).all())
    out = sliding.finish_torch(acc, ws)
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    one = sliding.blend_tiles_torch(_tiles(dims, T, stride, N, K, 0, ones=True), torch.zeros((N,) + dims + (K,)),
                                    T, stride, blend)
    assert torch.equal(one, ws[None, ..., None].expand_as(one))
    assert torch.equal(sliding.finish_torch(one, ws), torch.ones_like(one))


def test_constant_blend_of_a_tile_sized_image_is_the_tile():
    for T in ((1, 32, 32), (8, 8, 8)):
        p = _tiles(T, T, sliding.strides(T, 0.5), 3, 2, 11)
        acc = sliding.blend_tiles_torch(p, torch.zeros((3,) + T + (2,)), T, sliding.strides(T, 0.5), "constant")
        assert torch.equal(sliding.finish_torch(acc, sliding.weight_sum(T, T, sliding.strides(T, 0.5), "constant")), p)

    def f(t):
        return torch.sigmoid(t[..., :2] * 1.7)
    x = torch.randn(5, 32, 32, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(sliding.sliding_predict_torch(f, x, (1, 32, 32), 2, 0.5, "constant"), f(x))


@pytest.mark.parametrize("dims,T,stride", [g for g in GPU_GEOMETRIES if g[0][0] == 1][:4] +
                         [((10, 8, 12), (8, 8, 8), (4, 4, 4))])
@pytest.mark.parametrize("blend", sliding.BLENDS)
def test_tile_order_equals_per_pixel_ascending_order(dims, T, stride, blend):
    """What the output-centric kernel does: every pixel adds its covering tiles in ascending
    tile index, one multiplication and one addition each, from the accumulator's old value."""
    N, K = 2, 2
    p = _tiles(dims, T, stride, N, K, 5)
    w = sliding.weight_map(T, blend)
    acc0 = torch.randn((N,) + dims + (K,), generator=torch.Generator().manual_seed(6))
    want = sliding.blend_tiles_torch(p, acc0.clone(), T, stride, blend)
    tl = sliding.tile_list(dims, T, stride)
    got = acc0.clone().numpy()
    pn, wn = p.numpy(), w.numpy()
    for n in range(N):
        for d in range(dims[0]):
            for h in range(dims[1]):
                for x in range(dims[2]):
                    a = got[n, d, h, x].copy()
                    for r, (od, oh, ow) in enumerate(tl):
                        if od <= d < od + T[0] and oh <= h < oh + T[1] and ow <= x < ow + T[2]:
                            prod = (wn[d - od, h - oh, x - ow] * pn[n * len(tl) + r, d - od, h - oh, x - ow]).astype(
                                np.float32)
                            a = (a + prod).astype(np.float32)
                    got[n, d, h, x] = a
    assert np.array_equal(got, want.numpy())
    # batches issued one by one give the same bits as all tiles at once
    acc = acc0.clone()
    for t0 in range(0, p.shape[0], 3):
        sliding.blend_tiles_torch(p[t0:t0 + 3], acc, T, stride, blend, t0)
    assert torch.equal(acc, want)


def test_extract_slots_and_zero_padding():
    T, stride = (1, 32, 32), (1, 16, 16)
    x = torch.randn(3, 40, 56, 4, generator=torch.Generator().manual_seed(1))
    tl = sliding.tile_list((1, 40, 56), T, stride)
    assert len(tl) == 6 and [o[1:] for o in tl] == [(0, 0), (0, 16), (0, 24), (8, 0), (8, 16), (8, 24)]
    b = sliding.extract_tiles_torch(x, T, stride, 4, 16, 2)
    assert tuple(b.shape) == (4, 1, 32, 32, 4)
    assert torch.equal(b[0, 0], x[2, 8:40, 16:48]) and torch.equal(b[1, 0], x[2, 8:40, 24:56])
    assert not b[2:].any()
    small = sliding.extract_tiles_torch(x[:, :24], T, stride, 4, 0, 3)      # H smaller than the tile
    assert torch.equal(small[1, 0, :24], x[0, :24, 16:48]) and not small[:, :, 24:].any() and not small[3].any()
    with pytest.raises(ValueError):
        sliding.extract_tiles_torch(x, T, stride, 4, 16, 3)


# ------------------------------------------------------------------ the whole loop
def _pointwise(t):
    return torch.sigmoid(t[..., :2] * 1.3 + 0.1)


def _ulps(out, want):
    return (out - want).abs().double() / torch.from_numpy(np.spacing(want.numpy())).double()


@pytest.mark.parametrize("case", [
    # every pixel in one tile: any weight map
    dict(shape=(3, 64, 96, 4), T=(1, 32, 32), overlap=0.0, blend="gaussian"),
    dict(shape=(3, 64, 96, 4), T=(1, 32, 32), overlap=0.0, blend="constant"),
    dict(shape=(2, 20, 24, 4), T=(1, 32, 32), overlap=0.5, blend="gaussian"),         # smaller than the tile
    dict(shape=(1, 16, 16, 32, 4), T=(16, 16, 16), overlap=0.0, blend="gaussian"),
    # constant weights, 1, 2 or 4 covering tiles (the image is the tile plus whole strides)
    dict(shape=(3, 48, 80, 4), T=(1, 32, 32), overlap=0.5, blend="constant"),
], ids=lambda c: "%s-%s-%g" % ("x".join(map(str, c["shape"][1:-1])), c["blend"], c["overlap"]))
def test_sliding_predict_reproduces_a_pointwise_function_within_2_ulp(case):
    x = torch.randn(case["shape"], generator=torch.Generator().manual_seed(3))
    for B in (4, 5):                        # (a last batch with empty slots, and none)
        out = sliding.sliding_predict_torch(_pointwise, x, case["T"], B, case["overlap"], case["blend"])
        want = _pointwise(x)
        assert out.shape == want.shape and out.dtype == torch.float32
        u = _ulps(out, want)
        print("sliding pointwise", case, "max ulp", float(u.max()))
        assert float(u.max()) <= 2.0


@pytest.mark.parametrize("case", [
    dict(shape=(3, 40, 56, 4), T=(1, 32, 32), overlap=0.5, blend="gaussian"),
    dict(shape=(3, 40, 56, 4), T=(1, 32, 32), overlap=0.75, blend="gaussian"),
    dict(shape=(3, 40, 56, 4), T=(1, 32, 32), overlap=0.75, blend="constant"),
    dict(shape=(1, 20, 16, 24, 4), T=(16, 16, 16), overlap=0.5, blend="gaussian"),
], ids=lambda c: "%s-%s-%g" % ("x".join(map(str, c["shape"][1:-1])), c["blend"], c["overlap"]))
def test_sliding_predict_of_a_pointwise_function_meets_the_per_pixel_bound(case):
    """n covering tiles: |out - p| <= (3 n - 1) 2^-24 p to first order (module docstring); these
    geometries reach 4 to 5 ulp, so the 2 ulp of a single tile cannot hold for them."""
    x = torch.randn(case["shape"], generator=torch.Generator().manual_seed(4))
    T = case["T"]
    out = sliding.sliding_predict_torch(_pointwise, x, T, 4, case["overlap"], case["blend"])
    want = _pointwise(x)
    dims = tuple(x.shape[1:-1]) if x.dim() == 5 else (1,) + tuple(x.shape[1:-1])
    n = sliding.weight_sum(dims, T, sliding.strides(T, case["overlap"]), "constant").view(x.shape[1:-1])
    bound = ((3 * n - 1) * EPS * (1 + 1e-5))[None, ..., None].double() * want.double()
    err = (out.double() - want.double()).abs()
    print("sliding pointwise", case, "max ulp", float(_ulps(out, want).max()), "max err / bound",
          float((err / bound).max()), "max n", int(n.max()))
    assert bool((err <= bound).all())


def test_torch_backend_and_predictor_sliding(tmp_path):
    """`TorchBackend.predict_sliding` is the oracle around its own `predict`; the Predictor works
    in chunks of whole images under the byte cap, tile numbering restarting per chunk, and
    `tta=` composes."""
    from unet_distributed_amd.inference import Predictor
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import UNetSpec
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    from unet_distributed_amd.runtime.params import FlatParams
    spec = UNetSpec(in_channels=2, n_cl_out=2, base=8, depth=2, use_upsampling=True, dims=2, dropout=0.0)
    flat = FlatParams(spec, device="cpu")
    flat.load_dict(reference.init_params(spec, seed=4))
    rs = np.random.RandomState(0)
    x = rs.randn(5, 20, 28, 2).astype(np.float32)
    y = (rs.rand(5, 20, 28, 2) > 0.5).astype(np.float32)
    for tta in ("", "flip"):
        model = Predictor(spec, flat, 16, "cpu", batch=3, tta=tta)
        per = 20 * 28 * 4 * 4
        assert model.sliding_chunks(x.shape, 2 * per) == [(0, 2), (2, 4), (4, 5)]
        assert model.sliding_chunks(x.shape, 1) == [(i, i + 1) for i in range(5)]
        assert model.sliding_chunks(x.shape) == [(0, 5)]
        got = model.predict_sliding(x, overlap=0.5, blend="gaussian", max_bytes=2 * per)
        want = torch.cat([sliding.sliding_predict_torch(model.backend.predict, torch.from_numpy(x[s:t]), (1, 16, 16),
                                                        3, 0.5, "gaussian") for s, t in ((0, 2), (2, 4), (4, 5))])
        assert got.shape == (5, 20, 28, 2) and np.array_equal(got, want.numpy())
        assert 0.0 <= got.min() and got.max() <= 1.0
        st = model.stats_sliding(x, y, 0.5, max_bytes=2 * per)
        assert np.array_equal(st, case_stats_torch(want, torch.from_numpy(y), 0.5).double().numpy())
        sf = model.surface_sliding(x, y, 0.5, max_bytes=2 * per)
        assert sf.dtype == np.int64
        assert np.array_equal(sf, case_surface_torch(want, torch.from_numpy(y), 0.5).long().numpy())
    plain = Predictor(spec, flat, 16, "cpu", batch=3)
    xs = x[:, :16, :16]
    assert np.array_equal(plain.predict_sliding(xs, blend="constant"), plain.predict(xs))
    with pytest.raises(ValueError, match="0.8"):
        plain.predict_sliding(x, overlap=0.8)
    with pytest.raises(ValueError, match="'linear'"):
        plain.predict_sliding(x, blend="linear")
    with pytest.raises(ValueError, match="shape"):
        plain.predict_sliding(x[..., :1])


# ------------------------------------------------------------------ static plan validation
ENGINES = [
    dict(out_channels=1, batch_size=4, img_size=32, in_channels=4),
    dict(out_channels=3, batch_size=1, img_size=32, in_channels=4),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp16"),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dtype="fp32"),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=4, dims=3),
    dict(out_channels=1, batch_size=2, img_size=32, in_channels=1, norm="batch"),
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
def test_dry_run_engines_expose_sliding_to_plan_check(kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.runtime.plan_check import check_engine, check_sliding_plan
    cfg = Config(**kw)
    e = _dry_engine(cfg)
    # nothing is planned or allocated until it is asked for, and the finding says so
    assert e.sw_plan is None and not hasattr(e, "sw_x")
    assert check_sliding_plan(e) != []
    names = (e.plan.names(), e.eval_plan.names())
    e.plan_sliding()
    B = cfg.batch_size
    want = ["sw_extract:0", "sw_blend:0", "sw_finish"] if B >= 2 else \
        ["sw_extract:0", "sw_blend:0", "sw_extract:1", "sw_blend:1", "sw_finish"]
    assert e.sw_plan.names() == want
    assert check_sliding_plan(e) == []
    assert (e.plan.names(), e.eval_plan.names()) == names and check_engine(e) == {"train": [], "eval": []}
    d, h, w = e.sdims(1)
    assert e.sw_x.numel() == B * d * h * w * cfg.in_channels and e.sw_x.dtype == torch.float32
    assert tuple(e.sw_w.shape) == (2, d, h, w)
    assert torch.equal(e.sw_w[0], torch.ones(d, h, w))
    assert torch.equal(e.sw_w[1], sliding.weight_map((d, h, w), "gaussian"))
    with pytest.raises(RuntimeError):
        e.predict_sliding(torch.zeros((1,) + (40,) * cfg.dims + (cfg.in_channels,)))   # validated, never launched
    # a shrunk accumulator or staging batch is a named finding
    acc, xb = e.sw_acc, e.sw_x
    e.sw_acc = acc.view(-1)[:-4]
    errs = check_sliding_plan(e)
    assert errs and any("sw_blend" in m and "past its end" in m for m in errs)
    assert any("sw_finish" in m and "past its end" in m for m in errs)
    e.sw_acc, e.sw_x = acc, xb.view(-1)[:-4]
    errs = check_sliding_plan(e)
    assert errs and "sw_extract" in errs[0] and "past its end" in errs[0]
    e.sw_x = xb
    assert check_sliding_plan(e) == []


def test_generic_ops_refuse_bad_arguments_at_plan_time():
    from unet_distributed_amd import native
    C = native.require()
    x, xb = torch.zeros(3 * 40 * 56 * 4), torch.zeros(4 * 32 * 32 * 4)
    w, ws = torch.zeros(32 * 32), torch.zeros(40 * 56)
    px, pxb, pw, pws = (int(t.data_ptr()) for t in (x, xb, w, ws))
    #       N  D  H   W   C  Td Th  Tw  sd sh  sw  B  t0 nt
    ok = [3, 1, 40, 56, 4, 1, 32, 32, 1, 16, 16, 4, 16, 2]
    plan = C.Plan(0)
    plan.add_generic("sw_extract", [px, pxb], ok, [], "ok")
    plan.add_generic("sw_blend", [pxb, pw, px], ok, [], "ok")
    plan.add_generic("sw_extract", [px, pxb], ok[:4] + [7] + ok[5:], [], "any C")
    plan.add_generic("sw_finish", [px, pws], [3, 1, 40, 56, 4], [], "ok")
    n0 = plan.size()

    def put(i, v):
        return ok[:i] + [v] + ok[i + 1:]
    bad = [put(4, 0), put(0, 0), put(2, 0), put(6, 0),
           put(9, 7), put(9, 33), put(10, 0), put(8, 2),          # a stride outside [T / 4, T]
           put(12, -1), put(13, 0), put(13, 5), put(12, 17),      # t0 / nt outside the batch and the grid
           put(11, 1 << 19),                                      # B Td Th Tw C = 2^31
           put(0, 1 << 31)]
    for ints in bad:
        for kind, ptrs in (("sw_extract", [px, pxb]), ("sw_blend", [pxb, pw, px])):
            with pytest.raises(ValueError):
                plan.add_generic(kind, ptrs, ints, [], "bad")
            with pytest.raises(ValueError):
                C.generic(kind, ptrs, ints, [], 0)                # (immediate style: nothing launched)
    for K in (0, 5):
        with pytest.raises(ValueError, match="classes"):
            plan.add_generic("sw_blend", [pxb, pw, px], put(4, K), [], "bad K")
        with pytest.raises(ValueError, match="classes"):
            plan.add_generic("sw_finish", [px, pws], [3, 1, 40, 56, K], [], "bad K")
    # the images of one batch: 2^31 floats
    with pytest.raises(ValueError, match="2\\^31"):
        plan.add_generic("sw_blend", [pxb, pw, px], [1, 1, 1 << 15, 1 << 14, 4, 1, 32, 32, 1, 16, 16, 4, 0, 2], [],
                         "big")
    with pytest.raises(ValueError, match="2\\^31"):
        plan.add_generic("sw_finish", [px, pws], [1 << 9, 1, 1024, 1024, 4], [], "big")
    for kind, ptrs in (("sw_extract", [px, pxb]), ("sw_blend", [pxb, pw, px])):
        for null in range(len(ptrs)):
            p = list(ptrs)
            p[null] = 0
            with pytest.raises(ValueError):
                plan.add_generic(kind, p, ok, [], "null")
            p[null] = ptrs[null] + 2
            with pytest.raises(ValueError):
                plan.add_generic(kind, p, ok, [], "odd")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, ok[:13], [], "short")
    for p in ([0, pws], [px, 0], [px + 1, pws]):
        with pytest.raises(ValueError):
            plan.add_generic("sw_finish", p, [3, 1, 40, 56, 4], [], "bad")
    assert plan.size() == n0
    assert plan.check_dispatch(0, n0) == []


def test_plan_check_extents_follow_the_touched_images():
    from unet_distributed_amd.runtime.plan_check import _generic_rw, _generic_write_spans
    ints = [3, 1, 40, 56, 4, 1, 32, 32, 1, 16, 16, 4, 0, 4]
    assert _generic_write_spans("sw_extract", [100, 200], ints) == [(200, 4 * 32 * 32 * 4 * 4)]
    img = 40 * 56 * 3 * 4
    for t0, nt, last in ((0, 4, 0), (4, 4, 1), (8, 4, 1), (12, 4, 2), (16, 2, 2)):
        got = _generic_write_spans("sw_blend", [1, 2, 300], ints[:4] + [3] + ints[5:12] + [t0, nt])
        assert got == [(300, (last + 1) * img)], (t0, got)
    assert _generic_write_spans("sw_finish", [300, 400], [3, 1, 40, 56, 3]) == [(300, 3 * img)]
    assert _generic_rw("sw_blend", [1, 2, 3], ints) == ([1, 2, 3], [3])
    assert _generic_rw("sw_extract", [1, 2], ints) == ([1], [2])
    assert _generic_rw("sw_finish", [1, 2], ints) == ([1, 2], [1])


# ------------------------------------------------------------------ command line
def test_sanity_check_sliding_on_the_cpu(tmp_path, capsys):
    from unet_distributed_amd import sanity_check
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.ops.losses import sanity_dice
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, out_channels=2, depth=2, base_filters=8, checkpoint_dir=str(tmp_path))
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    export = export_model(cfg, spec, flat)
    argv = ["--export_dir", export, "--device", "cpu", "--backend", "torch", "--batch_size", "4", "--all_batches",
            "--synthetic", "6", "--synthetic_size", "48"]
    avg = sanity_check.main(argv + ["--sliding", "--per_class", "--hd95"])
    out = capsys.readouterr().out
    assert "Average Dice for Test Set = " in out and "class 1: case Dice = " in out
    assert "Case Dice = " in out and "(6 cases)" in out and "class 1: HD95 = " in out and "HD95 = " in out
    x, y = synthetic_brats(6, 48, 4, 2, seed=1, out_channels=2)
    assert x.shape == (6, 48, 48, 4)
    model = load_saved_model(export, device="cpu", batch=4, backend="torch")
    want = np.mean([sanity_dice(y[s:s + 4], model.predict_sliding(x[s:s + 4])) for s in (0, 4)])
    assert abs(avg - want) < 1e-12
    other = sanity_check.main(argv + ["--sliding", "--overlap", "0.25", "--blend", "constant"])
    assert other != avg
    # --sliding covers every sample with or without --all_batches
    assert sanity_check.main([v for v in argv if v != "--all_batches"] + ["--sliding"]) == avg
    # a size other than the model's needs --sliding; a bad overlap is an argparse error naming it
    for extra in ([], ["--sliding", "--overlap", "0.8"]):
        with pytest.raises(SystemExit):
            sanity_check.main(argv + extra)
    assert "0.8" in capsys.readouterr().err
    # without the flags nothing changes
    a = sanity_check.main(argv[:-2])
    b = sanity_check.main(argv[:-2] + ["--synthetic_size", "32"])
    assert a == b

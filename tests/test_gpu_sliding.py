"""Sliding-window inference on the GPU (csrc/kernels/sliding.h): sw_extract against
`extract_tiles_torch`, sw_blend + sw_finish against `blend_tiles_torch` / `finish_torch`, the
executors' `predict_sliding` bit for bit against a manual loop through the same executor, and
the public paths (`Predictor.predict_sliding`, `stats_sliding`, `surface_sliding`).

Exactness: the extraction is a copy; the blend adds each pixel's covering tiles in ascending
tile order with one fp32 multiplication and one fp32 addition each (never an fma) and the finish
is one correctly rounded division -- the arithmetic of `ops.sliding` on the same device -- so
every comparison is `torch.equal`.  Bound of the fp32 statistics sums: n non-negative fp32 terms
added in any order are within n 2^-24 of the exact sum, relative (tests/test_gpu_seg_stats.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PAD = 64

# (N, image dims, tile, stride, B): tile 32, 6 tiles per 40 x 56 image at stride 16 -- 18 tiles, 4 full
# batches and one of 2, both axes with a clamped last tile; 24 x 72: H smaller than the tile
GEO_2D = [(3, (1, 40, 56), (1, 32, 32), (1, s, s), 4) for s in (16, 32, 8)] + \
         [(3, (1, 24, 72), (1, 32, 32), (1, s, s), 4) for s in (16, 32, 8)]
GEO_3D = (2, (40, 32, 48), (32, 32, 32), (16, 16, 16), 2)


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _guarded(n, dev, off=0, fill=float("nan")):
    """(whole allocation, the n floats inside it) with PAD NaN floats on either side; `off`:
    floats by which the inside is moved off its 16-byte alignment."""
    big = torch.full((n + 2 * PAD + off,), fill, dtype=torch.float32, device=dev)[off:]
    big[:PAD] = float("nan")
    big[PAD + n:] = float("nan")
    return big, big[PAD:PAD + n]


def _guard_ok(big, n):
    return bool(torch.isnan(big[:PAD]).all() and torch.isnan(big[PAD + n:]).all())


def _ints(N, dims, CK, T, stride, B, t0, nt):
    return [N] + list(dims) + [CK] + list(T) + list(stride) + [B, t0, nt]


# ------------------------------------------------------------------ sw_extract
def _extract_case(dev, geo, Cin, off=0):
    from unet_distributed_amd.ops import sliding
    N, dims, T, stride, B = geo
    g = torch.Generator().manual_seed(100 * Cin + dims[1] + stride[1])
    x = torch.randn((N,) + dims + (Cin,), generator=g).to(dev)
    if off:                                 # (x too sits `off` floats past a 16-byte boundary)
        x = torch.cat([x.new_zeros(off), x.reshape(-1)])[off:].view(x.shape)
        assert x.data_ptr() % 16 == 4 * off
    total = N * sliding.tiles_per_image(dims, T, stride)
    n = B * T[0] * T[1] * T[2] * Cin
    seen = 0
    for t0 in range(0, total, B):
        nt = min(B, total - t0)
        tag = "C%d %r stride %r off %d t0 %d" % (Cin, dims, stride, off, t0)
        big, xb = _guarded(n, dev, off)
        C().generic("sw_extract", [ptr(x), ptr(xb)], _ints(N, dims, Cin, T, stride, B, t0, nt), [], stream())
        torch.cuda.synchronize()
        assert _guard_ok(big, n), tag + ": wrote outside the staging batch"
        got = xb.view((B,) + T + (Cin,))
        assert not torch.isnan(got).any(), tag + ": a slot or a position past the image was left unwritten"
        assert torch.equal(got, sliding.extract_tiles_torch(x, T, stride, B, t0, nt)), tag
        if nt < B:
            assert not got[nt:].any(), tag + ": the slots past the last tile must be zeros"
        seen += nt
    assert seen == total
    return total


@pytest.mark.parametrize("Cin", [1, 4])
def test_sw_extract_matches_extract_tiles_torch_2d(cuda_dev, Cin):
    for geo in GEO_2D:
        total = _extract_case(cuda_dev, geo, Cin)
        if geo[1] == (1, 40, 56) and geo[3] == (1, 16, 16):
            assert total == 18                     # 4 full batches and one of 2: slots 2 and 3 zeros
    # a base 4 bytes off the 16-byte alignment: the float path
    _extract_case(cuda_dev, GEO_2D[0], Cin, off=1)
    _extract_case(cuda_dev, GEO_2D[3], Cin, off=1)


@pytest.mark.parametrize("Cin,W", [(1, 54), (2, 54), (3, 56), (3, 55), (4, 55)])
def test_sw_extract_rows_that_are_not_whole_vectors(cuda_dev, Cin, W):
    """W C % 4 != 0 (row starts off the vector grid) takes the float path; C = 3 with W = 56 has
    whole vectors that straddle pixels."""
    _extract_case(cuda_dev, (3, (1, 40, W), (1, 32, 32), (1, 16, 16), 4), Cin)
    _extract_case(cuda_dev, (2, (1, 40, W), (1, 32, 32), (1, 8, 8), 5), Cin)


def test_sw_extract_matches_extract_tiles_torch_3d(cuda_dev):
    assert _extract_case(cuda_dev, GEO_3D, 4) == 8
    # D smaller than the tile, a clamped last tile on D, H and W
    _extract_case(cuda_dev, (2, (20, 40, 36), (32, 32, 32), (16, 16, 16), 3), 1)
    _extract_case(cuda_dev, (1, (40, 36, 44), (32, 32, 32), (8, 8, 8), 3), 4)


# ------------------------------------------------------------------ sw_blend + sw_finish
def _blend_case(dev, geo, K, blend, ones=False):
    from unet_distributed_amd.ops import sliding
    N, dims, T, stride, B = geo
    tpi = sliding.tiles_per_image(dims, T, stride)
    total = N * tpi
    g = torch.Generator().manual_seed(10 * K + dims[1] + stride[1])
    tiles = torch.ones((total,) + T + (K,)) if ones else torch.rand((total,) + T + (K,), generator=g)
    tiles = tiles.to(dev)
    w = sliding.weight_map(T, blend).to(dev)
    wsum = sliding.weight_sum(dims, T, stride, blend).to(dev)
    acc0 = (torch.zeros((N,) + dims + (K,)) if ones else torch.randn((N,) + dims + (K,), generator=g)).to(dev)
    n = acc0.numel()
    tag = "K%d %r stride %r %s" % (K, dims, stride, blend)
    runs = []
    for _ in range(2):
        big, acc = _guarded(n, dev)
        acc.copy_(acc0.reshape(-1))
        want = acc0.clone()
        for t0 in range(0, total, B):
            nt = min(B, total - t0)
            prob = torch.full((B,) + T + (K,), float("nan"), device=dev)     # (slots >= nt are never read)
            prob[:nt] = tiles[t0:t0 + nt]
            before = acc.clone().view(acc0.shape)
            C().generic("sw_blend", [ptr(prob), ptr(w), ptr(acc)], _ints(N, dims, K, T, stride, B, t0, nt), [],
                        stream())
            torch.cuda.synchronize()
            assert _guard_ok(big, n), tag + ": wrote outside acc"
            sliding.blend_tiles_torch(tiles[t0:t0 + nt], want, T, stride, blend, t0, w=w)
            got = acc.view(acc0.shape)
            assert torch.equal(got, want), tag + " t0 %d" % t0
            lo, hi = t0 // tpi, (t0 + nt - 1) // tpi
            assert torch.equal(got[:lo], before[:lo]) and torch.equal(got[hi + 1:], before[hi + 1:]), \
                tag + ": an image the batch does not touch changed"
        C().generic("sw_finish", [ptr(acc), ptr(wsum)], [N] + list(dims) + [K], [], stream())
        torch.cuda.synchronize()
        assert _guard_ok(big, n), tag + ": the finish wrote outside acc"
        out = acc.clone().view(acc0.shape)
        assert torch.equal(out, sliding.finish_torch(want, wsum)), tag + ": finish"
        runs.append(out)
    assert torch.equal(runs[0], runs[1]), tag + ": two runs differ"
    if ones:
        assert torch.equal(runs[0], torch.ones_like(runs[0])), tag + ": p == 1 must give exactly 1"
    return runs[0]


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sw_blend_and_finish_match_the_oracle_2d(cuda_dev, K):
    for geo in GEO_2D:
        for blend in ("constant", "gaussian"):
            _blend_case(cuda_dev, geo, K, blend)
    for blend in ("constant", "gaussian"):
        _blend_case(cuda_dev, GEO_2D[0], K, blend, ones=True)
        _blend_case(cuda_dev, GEO_2D[5], K, blend, ones=True)
    # odd sizes, a batch that spans three images (B = 9 > 4 tiles per image)
    _blend_case(cuda_dev, (4, (1, 37, 45), (1, 32, 32), (1, 16, 16), 9), K, "gaussian")


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sw_blend_and_finish_match_the_oracle_3d(cuda_dev, K):
    for blend in ("constant", "gaussian"):
        _blend_case(cuda_dev, GEO_3D, K, blend)
    _blend_case(cuda_dev, GEO_3D, K, "gaussian", ones=True)
    _blend_case(cuda_dev, (1, (20, 40, 36), (32, 32, 32), (8, 16, 32), 3), K, "gaussian")


def test_sw_blend_rows_longer_than_a_workgroup_piece(cuda_dev):
    """W K = 1100 > 1024 floats: a row is split over two workgroups along W."""
    _blend_case(cuda_dev, (1, (1, 33, 275), (1, 32, 32), (1, 16, 16), 7), 4, "gaussian")


# ------------------------------------------------------------------ executors
def _backend(cuda_dev, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(**kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=cuda_dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    nb = NativeBackend(spec, flat, cfg, cuda_dev, cfg.batch_size)
    nb.engine.repack()
    return nb, cfg


def _images(cfg, n, seed, dev):
    sp = (40, 56) if cfg.dims == 2 else (40, 32, 48)
    return torch.randn((n,) + sp + (cfg.in_channels,), generator=torch.Generator().manual_seed(seed)).to(dev)


def _manual(nb, x, T, overlap, blend):
    """The oracle: python-sliced tiles in the same slot order, `backend.predict` per batch (the
    same executor's plain load and evaluation plan, or its TTA), the blend and division in torch."""
    from unet_distributed_amd.ops import sliding
    return sliding.sliding_predict_torch(nb.predict, x, T, nb.B, overlap, blend)


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
def test_predict_sliding_is_bit_exact_against_a_manual_loop(cuda_dev, kw):
    from unet_distributed_amd.ops import sliding
    from unet_distributed_amd.runtime.plan_check import check_sliding_plan
    nb, cfg = _backend(cuda_dev, **kw)
    e = nb.engine
    assert e.sw_plan is None                                       # nothing planned until it is used
    T = sliding.tile_shape(32, cfg.dims)
    x = _images(cfg, 3 if cfg.dims == 2 else 2, 5, cuda_dev)
    for overlap, blend in ((0.5, "gaussian"), (0.25, "constant")):
        want = _manual(nb, x, T, overlap, blend)
        got = nb.predict_sliding(x, overlap, blend).clone()
        torch.cuda.synchronize()
        assert got.shape == x.shape[:-1] + (cfg.out_channels,) and got.dtype == torch.float32
        assert torch.equal(got, want), (overlap, blend)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        assert torch.equal(nb.predict_sliding(x, overlap, blend), got), "two runs differ"
    assert check_sliding_plan(e) == []
    # blend = constant on one batch of images of exactly the tile size: the plain prediction
    sp = (slice(None),) + (slice(0, 32),) * cfg.dims
    xs = torch.cat([x[sp], x[sp]])[:nb.B].contiguous()
    assert torch.equal(nb.predict_sliding(xs, 0.5, "constant"), nb.predict(xs))
    with pytest.raises(ValueError, match="0.9"):
        nb.predict_sliding(x, 0.9, "gaussian")
    with pytest.raises(ValueError, match="'cosine'"):
        nb.predict_sliding(x, 0.5, "cosine")
    with pytest.raises(ValueError, match="shape"):
        nb.predict_sliding(x[..., :2], 0.5, "gaussian")


@pytest.mark.parametrize("kw", [ENGINE_CASES[1], ENGINE_CASES[3], ENGINE_CASES[5]], ids=lambda kw: "K%d-%s-%dd" % (
    kw["out_channels"], kw.get("dtype", "bf16"), kw.get("dims", 2)))
def test_predict_sliding_composes_with_tta(cuda_dev, kw):
    from unet_distributed_amd.ops import sliding
    nb, cfg = _backend(cuda_dev, eval_tta="flip", **kw)
    assert len(nb.tta) == (8 if cfg.dims == 3 else 4)
    T = sliding.tile_shape(32, cfg.dims)
    x = _images(cfg, 2 if cfg.dims == 2 else 1, 6, cuda_dev)
    want = _manual(nb, x, T, 0.5, "gaussian")
    got = nb.predict_sliding(x, 0.5, "gaussian")
    assert torch.equal(got, want)
    off, _ = _backend(cuda_dev, **kw)
    assert not torch.equal(off.predict_sliding(x, 0.5, "gaussian"), got)     # (the network is not equivariant)


def test_ops_of_predict_sliding(cuda_dev, monkeypatch):
    """One call issues, per batch of tiles, sw_extract, the plain gather and the evaluation plan,
    sw_blend; one sw_finish at the end; `predict` issues none of them."""
    nb, cfg = _backend(cuda_dev, out_channels=1, batch_size=4, img_size=32, in_channels=4)
    issued = []
    real = nb.engine.C.generic

    class Spy:
        def __init__(self, mod):
            self._mod = mod

        def generic(self, kind, *a, **k):
            issued.append(kind)
            return real(kind, *a, **k)

        def __getattr__(self, name):
            return getattr(self._mod, name)
    monkeypatch.setattr(nb.engine, "C", Spy(nb.engine.C))
    x = _images(cfg, 3, 7, cuda_dev)
    xs = x[:, :32, :32].contiguous()
    nb.predict(torch.cat([xs, xs[:1]]))
    assert issued == ["gather_batch"] and nb.engine.sw_plan is None
    del issued[:]
    nb.predict_sliding(x, 0.5, "gaussian")
    torch.cuda.synchronize()
    assert issued == ["sw_extract", "gather_batch", "sw_blend"] * 5 + ["sw_finish"]


# ------------------------------------------------------------------ public paths
def _export(tmp_path, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.params import FlatParams
    from unet_distributed_amd.utils.checkpoint import export_model
    cfg = Config(img_size=32, in_channels=4, checkpoint_dir=str(tmp_path), **kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec)
    flat.load_dict(reference.init_params(spec, seed=3))
    return export_model(cfg, spec, flat)


def _check_stats(got, want, S, tag):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert torch.equal(got[..., 3:], want[..., 3:]), tag + ": counts"
    err = (got[..., :3] - want[..., :3]).abs()
    bound = S * EPS * want[..., :3].abs()
    print("sliding stats", tag, "max err / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), tag


@pytest.mark.parametrize("size", [(40, 56), (37, 45)], ids=lambda s: "%dx%d" % s)
def test_predictor_sliding_in_chunks_with_stats_and_surface(cuda_dev, tmp_path, size):
    """5 images under a byte cap that holds two: chunks (0, 2), (2, 4), (4, 5), tile numbering
    restarting per chunk.  37 x 45 = 1665 pixels is no multiple of 8: the statistics and surface
    ops refuse it and the torch fallback on the device scores it."""
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.ops import sliding
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    K = 3
    model = load_saved_model(_export(tmp_path, out_channels=K), device=cuda_dev, batch=4)
    assert model.name == "native"
    x, y = synthetic_brats(5, 64, 4, seed=2, out_channels=K)
    x = np.ascontiguousarray(x[:, :size[0], :size[1]])
    y = np.ascontiguousarray(y[:, :size[0], :size[1]]).astype(np.float32)
    S = size[0] * size[1]
    cap = 2 * S * (4 + K) * 4
    chunks = model.sliding_chunks(x.shape, cap)
    assert chunks == [(0, 2), (2, 4), (4, 5)]
    want = torch.cat([sliding.sliding_predict_torch(model.backend.predict, torch.from_numpy(x[s:t]).to(cuda_dev),
                                                    (1, 32, 32), 4, 0.5, "gaussian").cpu() for s, t in chunks])
    got = model.predict_sliding(x, max_bytes=cap)
    assert got.shape == (5,) + size + (K,) and got.dtype == np.float32
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(model.predict_sliding(x, max_bytes=cap), got), "two runs differ"
    whole = model.predict_sliding(x)                    # one chunk: other batches, the same tiles per image
    assert whole.shape == got.shape and np.array_equal(whole[:2], got[:2])
    yt = torch.from_numpy(y)
    st = model.stats_sliding(x, y, 0.5, max_bytes=cap)
    assert st.shape == (5, K, 6)
    _check_stats(st, case_stats_torch(want, yt, 0.5), S, "%dx%d" % size)
    sf = model.surface_sliding(x, y, 0.5, max_bytes=cap)
    assert sf.dtype == np.int64 and np.array_equal(sf, case_surface_torch(want, yt, 0.5).long().numpy())
    assert np.array_equal(model.surface_sliding(x, y, 0.5), sf)
    # the existing methods are what they were: a model-sized input goes through them unchanged
    xs = np.ascontiguousarray(x[:, :32, :32])
    assert np.array_equal(model.predict_sliding(xs, blend="constant"), model.predict(xs))
    with pytest.raises(ValueError, match="0.76"):
        model.predict_sliding(x, overlap=0.76)


def test_predictor_sliding_3d(cuda_dev, tmp_path):
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.ops import sliding
    from unet_distributed_amd.ops.seg_metrics import case_stats_torch, case_surface_torch
    model = load_saved_model(_export(tmp_path, out_channels=1, dims=3), device=cuda_dev, batch=2)
    assert model.name == "native"
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 40, 32, 48, 4, generator=g)
    y = torch.zeros(2, 40, 32, 48, 1)
    y[0, 10:30, 8:20, 12:40], y[1, 2:9, 20:32, 0:11] = 1.0, 1.0       # (blocks: the all-pairs oracle stays small)
    want = sliding.sliding_predict_torch(model.backend.predict, x.to(cuda_dev), (32, 32, 32), 2, 0.5, "gaussian")
    got = model.predict_sliding(x.numpy())
    assert np.array_equal(got, want.cpu().numpy())
    _check_stats(model.stats_sliding(x.numpy(), y.numpy()), case_stats_torch(want.cpu(), y, 0.5), 40 * 32 * 48, "3d")
    assert np.array_equal(model.surface_sliding(x.numpy(), y.numpy()),
                          case_surface_torch(want, y.to(cuda_dev), 0.5).long().numpy())


def test_sanity_check_sliding_on_the_native_backend(cuda_dev, tmp_path, capsys):
    from unet_distributed_amd import sanity_check
    export = _export(tmp_path, out_channels=2)
    avg = sanity_check.main(["--export_dir", export, "--batch_size", "4", "--all_batches", "--synthetic", "6",
                             "--synthetic_size", "48", "--sliding", "--per_class", "--hd95"])
    out = capsys.readouterr().out
    assert np.isfinite(avg) and "native backend" in out
    assert "class 1: case Dice = " in out and "(6 cases)" in out and "class 1: HD95 = " in out

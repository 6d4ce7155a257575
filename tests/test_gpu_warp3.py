"""3D rotation and zoom on the GPU: the trilinear batch gather (csrc/kernels/gather_resample.h, ops
gather_batch_warp3 / f32_gather_batch_warp3) against the definition in plain torch --
apply_torch(warp3_torch(index_select)) cast to the storage type, bit for bit: the geometry is
integer and every fp32 product and sum rounds on its own in both -- with and without an elastic
field, the intensity affine against float64 within one rounding, the in-plane warp and the crop
where the matrix leaves depth alone, device data outside its ranges against the oracle at the
clamped values, gather_check's refusals, the executors' load_indexed, the feeder's upload, and
one CLI run.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from unet_distributed_amd.data import augment as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 4096              # guard elements on each side of an output
NALL = 5                # samples of the resident dataset
ONE = 65536
# name: (torch dtype, op prefix, dtype id, unit roundoff of one rounding to the type)
TYPES = {"bf16": (torch.bfloat16, "", 0, 2.0 ** -8), "fp16": (torch.float16, "", 1, 2.0 ** -11),
         "fp32": (torch.float32, "f32_", 0, 2.0 ** -24)}
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr()) if t is not None else 0


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """An output of `n` elements in the middle of a NaN-filled buffer: after the launch the
    payload is finite and the guard regions are still NaN."""

    def __init__(self, n, dtype, dev):
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=dev)
        self.out = self.buf[PAD:PAD + n]

    def check(self):
        assert torch.isfinite(self.out.float()).all()
        assert torch.isnan(self.buf[:PAD].float()).all()
        assert torch.isnan(self.buf[PAD + self.out.numel():].float()).all()


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


@functools.lru_cache(maxsize=None)
def dataset(stored, cin, K):
    """The resident fp32 dataset of one stored shape (Ds, Hs, Ws), shared by the tests that read it
    and never written (randn: no negative zeros)."""
    g = torch.Generator().manual_seed(sum(stored) * 100 + 10 * cin + K)
    x = torch.randn((NALL,) + tuple(stored) + (cin,), generator=g)
    y = (torch.rand((NALL,) + tuple(stored) + (K,), generator=g) > 0.6).float()
    return x.cuda(), y.cuda()


def batch_idx(B, dev):
    """Unsorted sample indices out of NALL with repeats."""
    idx = [3, 2, 4, 2, 0, 1, 3, 4, 1, 0, 2, 4, 3, 1, 0, 2][:B]
    return torch.tensor(idx, dtype=torch.int64, device=dev)


def origins(B, stored, patch):
    """int32 [B][3]: 0, the maximum, odd values and mixtures, all inside [0, S - T]."""
    mx = [s - t for s, t in zip(stored, patch)]
    rows = [(0, 0, 0), tuple(mx), (1, 1, 3), (mx[0], 0, mx[2]), (0, mx[1], 0), (3, 5, 7), (mx[0] - 1, mx[1] - 1, 1),
            (1, mx[1], mx[2] - 1)]
    rows = [tuple(min(max(v, 0), m) for v, m in zip(r, mx)) for r in rows]
    return torch.tensor([rows[i % len(rows)] for i in range(B)], dtype=torch.int32)


def matrices(kind, B=16):
    """int32 [B][9].  `defaults`: draw_spatial3 at the flags' defaults (30 / 15 degrees, zoom a =
    0.25).  `axis30`: 30 and -30 degrees about each single axis, alone and at zooms 0.8 / 1.25 (with
    and without the depth zoom), then rows drawn at 30 degrees out of plane."""
    if kind == "defaults":
        m = A.draw_spatial3(11, 3, np.arange(B), "rotate3d,scale3d", 30.0, 15.0, 0.25)
    else:
        r = np.radians(30.0)
        rows = []
        for ax in range(3):
            for sign, z, zd in ((1, 1.0, 1.0), (-1, 0.8, 0.8), (1, 1.25, 1.0)):
                th = [0.0, 0.0, 0.0]
                th[ax] = sign * r
                rows.append(A.mat3_of(th[0], th[1], th[2], z, zd)[0])
        rows += list(A.draw_spatial3(5, 1, np.arange(B), "rotate3d,scale3d", 30.0, 30.0, 0.25))
        m = np.stack(rows[:B])
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32))


def fields(B, side, S):
    """int32 [B][N][N][2]: draw_elastic at the largest amplitude the flags admit (S / 8 pixels), one
    sample at the clamp's extremes and one all zero."""
    f = A.draw_elastic(7, 2, np.arange(B), side, S / 8.0, S)
    f[1, ::2], f[1, 1::2] = 1 << 22, -(1 << 22)
    f[2] = 0
    return torch.from_numpy(f)


def codes(B):
    code = torch.tensor([(3 * i + 5) % 16 for i in range(B)], dtype=torch.int32)        # every code, shuffled
    assert sorted(code.tolist()) == sorted(list(range(16)) * (B // 16))
    return code


def log2(S):
    return int(S).bit_length() - 1


def warp3_gather(x_all, y_all, idx, origin, code, mat, affine, field, S, tname, cpad, patch):
    """gather_batch_warp3 / f32_gather_batch_warp3 into guarded buffers; field None: a null pointer."""
    dt, pre, dt_id, _ = TYPES[tname]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    D, H, W = patch
    xb = Guarded(B * D * H * W * cpad, dt, x_all.device)
    tb = Guarded(B * D * H * W * K, dt, x_all.device)
    C().generic(pre + "gather_batch_warp3",
                [ptr(x_all), ptr(y_all), ptr(idx), ptr(origin), ptr(code), ptr(mat), ptr(affine), ptr(field),
                 ptr(xb.out), ptr(tb.out)],
                [B] + list(x_all.shape[1:4]) + [D, H, W, cin, cpad, K, log2(S) if field is not None else 0], [],
                stream(), dt_id)
    torch.cuda.synchronize()
    xb.check()
    tb.check()
    return xb.out.view((B,) + tuple(patch) + (cpad,)), tb.out.view((B,) + tuple(patch) + (K,))


def other_gather(which, x_all, y_all, idx, origin, code, mat, tname, cpad, patch):
    """gather_batch_warp (mat int32 [B][4]) or gather_batch_crop (mat None) at the same shape."""
    dt, pre, dt_id, _ = TYPES[tname]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    D, H, W = patch
    xb = torch.empty(B * D * H * W * cpad, dtype=dt, device=x_all.device)
    tb = torch.empty(B * D * H * W * K, dtype=dt, device=x_all.device)
    own = [ptr(origin), ptr(code)] + ([ptr(mat)] if which == "warp" else []) + [0]
    C().generic(pre + "gather_batch_" + which, [ptr(x_all), ptr(y_all), ptr(idx)] + own + [ptr(xb), ptr(tb)],
                [B] + list(x_all.shape[1:4]) + [D, H, W, cin, cpad, K], [], stream(), dt_id)
    torch.cuda.synchronize()
    return xb.view((B,) + tuple(patch) + (cpad,)), tb.view((B,) + tuple(patch) + (K,))


def oracle32(x_all, y_all, idx, origin, code, mat, field, S, patch):
    """apply_torch(warp3_torch(plain index_select)) in fp32, no affine."""
    x, y = A.warp3_torch(x_all.index_select(0, idx), y_all.index_select(0, idx), origin, patch, mat,
                         (field, S) if field is not None else None)
    return A.apply_torch(x, y, code if code is not None else np.zeros(idx.numel(), np.int32))


def oracle(x_all, y_all, idx, origin, code, mat, field, S, tname, cpad, patch):
    """... cast to the type, zero pad channels."""
    dt = TYPES[tname][0]
    x, y = oracle32(x_all, y_all, idx, origin, code, mat, field, S, patch)
    xb = torch.zeros(x.shape[:-1] + (cpad,), dtype=dt, device=x.device)
    xb[..., :x.shape[-1]] = x.to(dt)
    return xb, y.to(dt)


@functools.lru_cache(maxsize=None)
def shares(stored, patch, kind, B, null_origin, S):
    """The oracle's own masks of one geometry: it resamples an image and a target of ones, so a voxel
    reads 1 where all its taps are inside the stored volume and less where one is outside.  Returns
    (voxels with every tap inside, voxels with a tap outside, target voxels inside, outside)."""
    dev = torch.device("cuda")
    one = torch.ones((B,) + tuple(stored) + (1,), device=dev)
    org = None if null_origin else origins(B, stored, patch)
    x, y = A.warp3_torch(one, one, org, patch, matrices(kind, B), (fields(B, patch[-1], S), S) if S else None)
    return int((x == 1).sum()), int((x < 1).sum()), int((y == 1).sum()), int((y == 0).sum())


def cpad_of(tname, cin):
    return cin if tname == "fp32" else (4 if cin <= 4 else 8 if cin <= 8 else cin)


def check_warp3(dev, tname, stored, patch, kind, cin, K, S=0, B=16, null_origin=False):
    cpad = cpad_of(tname, cin)
    x_all, y_all = dataset(tuple(stored), cin, K)
    idx, code, mat = batch_idx(B, dev), codes(B), matrices(kind, B)
    org = None if null_origin else origins(B, stored, patch)
    dorg = None if null_origin else org.to(dev)
    field = fields(B, patch[-1], S) if S else None
    dfield = field.to(dev) if S else None
    # no case passes on zeros alone, or without a tap outside the volume
    assert all(v > 0 for v in shares(tuple(stored), tuple(patch), kind, B, null_origin, S)), (stored, patch, kind, S)
    wx, wt = oracle(x_all, y_all, idx, org, code, mat, field, S, tname, cpad, patch)
    gx, gt = warp3_gather(x_all, y_all, idx, dorg, code.to(dev), mat.to(dev), None, dfield, S, tname, cpad, patch)
    assert torch.equal(bits(gx), bits(wx)), (tname, stored, patch, kind, cin, cpad, K, S, "image")
    assert torch.equal(bits(gt), bits(wt)), (tname, stored, patch, kind, cin, cpad, K, S, "target")
    if cpad > cin:
        assert (gx[..., cin:] == 0).all()
    # two runs give the same bits
    hx, ht = warp3_gather(x_all, y_all, idx, dorg, code.to(dev), mat.to(dev), None, dfield, S, tname, cpad, patch)
    assert torch.equal(bits(gx), bits(hx)) and torch.equal(bits(gt), bits(ht))


# Cin 4 with K 1 and 3: the 16-byte tap loads; Cin 3: scalar taps padded to 4; Cin 5: Cpad 8 (fp32: 5, one
# lane per voxel); Cin 8: Cpad 8 with 16-byte taps; Cin 12: one lane per voxel
CHANNELS = [(4, 1), (4, 3), (3, 1), (5, 3), (8, 1), (12, 1)]
SHAPES = [((9, 40, 48), (5, 32, 32)), ((11, 56, 72), (6, 40, 40))]


@pytest.mark.parametrize("kind", ["defaults", "axis30"])
@pytest.mark.parametrize("stored,patch", SHAPES, ids=["whole-tiles", "ragged-tiles"])
@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_equals_warp3_torch(cuda_dev, tname, stored, patch, kind):
    """Patch (5, 32, 32) of (9, 40, 48): whole tiles in the plane, an odd depth; patch (6, 40, 40) of
    (11, 56, 72): tile edges that divide the patch in no direction.  All 16 codes."""
    for cin, K in CHANNELS:
        check_warp3(cuda_dev, tname, stored, patch, kind, cin, K)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_null_origin_on_samples_of_the_patch_size(cuda_dev, tname):
    """--augment rotate3d without --crop: every tap outside the patch is outside the volume."""
    for cin, K in ((4, 1), (3, 3), (8, 1), (12, 1)):
        check_warp3(cuda_dev, tname, (6, 32, 32), (6, 32, 32), "defaults", cin, K, null_origin=True)


@pytest.mark.parametrize("S", [8, 32])
@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_with_a_field(cuda_dev, tname, S):
    """The elastic displacement along (h, w) on top of the 3 x 3 matrix: the staged nodes of the tiled
    kernels and the global reads of the per-voxel one, at the smallest and the default cell."""
    for (stored, patch), kind in zip(SHAPES, ("axis30", "defaults")):
        for cin, K in ((4, 3), (3, 1), (5, 1), (12, 1)):
            check_warp3(cuda_dev, tname, stored, patch, kind, cin, K, S=S)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_intensity_within_one_rounding(cuda_dev, tname):
    """|out - r| <= 2 u |r| + 2^-22 (|scale v| + |shift|) + 2^-24 with r = scale v + shift in
    float64 and v the oracle's fp32 interpolation: one rounding to the storage type (unit
    roundoff u) with a factor-2 margin, plus the fp32 evaluation of the fma -- the bound of the
    warp gather's test, whose derivation holds unchanged: the affine acts on the oracle's fp32
    value.  The target is the geometry's alone."""
    dev = cuda_dev
    u = TYPES[tname][3]
    worst = 0.0
    stored, patch = SHAPES[1]
    for cin, K, S in ((4, 3, 0), (3, 1, 0), (12, 1, 0), (4, 1, 8), (8, 2, 32)):
        B = 16
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx, code, mat, org = batch_idx(B, dev), codes(B), matrices("defaults", B), origins(B, stored, patch)
        field = fields(B, patch[-1], S) if S else None
        dfield = field.to(dev) if S else None
        g = torch.Generator().manual_seed(cin + K)
        a = 0.25
        aff = torch.stack([1 - a + 2 * a * torch.rand(B, cin, generator=g),
                           -a + 2 * a * torch.rand(B, cin, generator=g)], dim=-1).contiguous()
        gx, gt = warp3_gather(x_all, y_all, idx, org.to(dev), code.to(dev), mat.to(dev), aff.to(dev), dfield, S, tname,
                              cpad, patch)
        _, t0 = warp3_gather(x_all, y_all, idx, org.to(dev), code.to(dev), mat.to(dev), None, dfield, S, tname, cpad,
                             patch)
        assert torch.equal(bits(gt), bits(t0))
        xg, _ = oracle32(x_all, y_all, idx, org, code, mat, field, S, patch)
        sh = (B, 1, 1, 1, cin)
        s, t = aff[..., 0].to(dev).double().view(sh), aff[..., 1].to(dev).double().view(sh)
        r = s * xg.double() + t
        bound = 2 * u * r.abs() + 2.0 ** -22 * ((s * xg.double()).abs() + t.abs()) + 2.0 ** -24
        err = (gx[..., :cin].double() - r).abs()
        worst = max(worst, float((err / bound).max()))
        print("intensity", tname, (cin, K, S), "max err / bound", float((err / bound).max()))
        assert (err <= bound).all(), (tname, cin, K, S)
        if cpad > cin:
            assert (gx[..., cin:] == 0).all()
    assert worst > 0


@pytest.mark.parametrize("tname", list(TYPES))
def test_matrices_that_leave_depth_alone_are_the_warp_and_the_crop_gather(cuda_dev, tname):
    """An embedded in-plane matrix == gather_batch_warp, with a field == gather_batch_elastic, and the
    identity == gather_batch_crop, bit for bit, with the same codes (fd = 0: s0 * 1 + s1 * 0)."""
    dev = cuda_dev
    stored, patch = SHAPES[1]
    for cin, K in ((4, 3), (3, 1), (8, 1), (12, 1)):
        B = 16
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx, code = batch_idx(B, dev), codes(B).to(dev)
        org = origins(B, stored, patch).to(dev)
        m2 = torch.from_numpy(A.draw_spatial(11, 3, np.arange(B), "rotate,scale", 30.0, 0.25))
        m3 = torch.from_numpy(A.embed_mat3(m2.numpy())).to(dev)
        a = warp3_gather(x_all, y_all, idx, org, code, m3, None, None, 0, tname, cpad, patch)
        b = other_gather("warp", x_all, y_all, idx, org, code, m2.to(dev), tname, cpad, patch)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), (tname, cin, "warp")
        assert (a[0].float() == 0).any() and (a[0].float() != 0).any()
        # strictly inside the volume: the crop
        mx = [s - t for s, t in zip(stored, patch)]
        ins = torch.tensor([[i % (mx[0] + 1), 1 + i % (mx[1] - 1), 1 + (3 * i) % (mx[2] - 1)] for i in range(B)],
                           dtype=torch.int32, device=dev)
        eye = torch.tensor([[ONE, 0, 0, 0, ONE, 0, 0, 0, ONE]] * B, dtype=torch.int32, device=dev)
        a = warp3_gather(x_all, y_all, idx, ins, code, eye, None, None, 0, tname, cpad, patch)
        b = other_gather("crop", x_all, y_all, idx, ins, code, None, tname, cpad, patch)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), (tname, cin, "crop")
        n = warp3_gather(x_all, y_all, idx, None, None, eye, None, None, 0, tname, cpad, patch)   # null origin and code
        z = warp3_gather(x_all, y_all, idx, torch.zeros_like(ins), torch.zeros_like(code), eye, None, None, 0, tname,
                         cpad, patch)
        assert torch.equal(bits(n[0]), bits(z[0])) and torch.equal(bits(n[1]), bits(z[1]))


def test_an_embedded_matrix_with_a_field_is_the_elastic_gather(cuda_dev):
    dev = cuda_dev
    stored, patch = SHAPES[0]
    for tname, cin, K, S in (("bf16", 4, 1, 8), ("fp16", 5, 2, 32), ("fp32", 4, 3, 8), ("bf16", 12, 1, 32)):
        dt, pre, dt_id, _ = TYPES[tname]
        B = 16
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx, code = batch_idx(B, dev), codes(B).to(dev)
        org = origins(B, stored, patch).to(dev)
        m2 = torch.from_numpy(A.draw_spatial(11, 3, np.arange(B), "rotate,scale", 30.0, 0.25))
        m3 = torch.from_numpy(A.embed_mat3(m2.numpy())).to(dev)
        field = fields(B, patch[-1], S).to(dev)
        a = warp3_gather(x_all, y_all, idx, org, code, m3, None, field, S, tname, cpad, patch)
        n = B * patch[0] * patch[1] * patch[2]
        xb, tb = torch.empty(n * cpad, dtype=dt, device=dev), torch.empty(n * K, dtype=dt, device=dev)
        m2d = m2.to(dev)
        C().generic(pre + "gather_batch_elastic",
                    [ptr(x_all), ptr(y_all), ptr(idx), ptr(org), ptr(code), ptr(m2d), 0, ptr(field), ptr(xb), ptr(tb)],
                    [B] + list(stored) + list(patch) + [cin, cpad, K, log2(S)], [], stream(), dt_id)
        torch.cuda.synchronize()
        assert torch.equal(bits(a[0].reshape(-1)), bits(xb)) and torch.equal(bits(a[1].reshape(-1)), bits(tb)), (tname, cin)


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_matrices_origins_and_fields_outside_their_ranges_are_clamped(cuda_dev, tname):
    """Matrix entries beyond +-2^18, origins outside the sample and field entries beyond +-2^22 (device
    data no launch can validate) read through the clamped values; every address stays inside the
    sample by the kernel's own clamps: tiled and per-voxel kernels."""
    dev = cuda_dev
    stored, patch = SHAPES[0]
    for cin, S in ((4, 8), (12, 32)):
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, 2)
        B = 8
        big = 1 << 20
        imax, imin = 2 ** 31 - 1, -2 ** 31
        wild_m = torch.tensor([[big, -big, big, -big, big, big, -big, big, big], [ONE, big, 0, -big, ONE, 0, 0, 0, ONE],
                               [imax, imin, imax, imin, imax, imin, imax, imin, imax], [imin] * 9, [imax] * 9,
                               [(1 << 18) + 1, 0, 0, 0, -(1 << 18) - 1, 0, 0, 0, ONE], [0, 0, big, 0, big, 0, -big, 0, 0],
                               matrices("defaults", 1)[0].tolist()], dtype=torch.int32)
        clamped_m = wild_m.clamp(-(1 << 18), 1 << 18)
        wild_o = torch.tensor([(-1, -1, -1), (0, -7, 1000), (5000, 9, -3), (imax, imax, imax), (imin, imin, imin),
                               (1, stored[1] - patch[1] + 1, 3), (0, 2, stored[2] - patch[2] + 1),
                               (stored[0] - patch[0] + 1, 0, 0)], dtype=torch.int32)
        mx = torch.tensor([s - t for s, t in zip(stored, patch)], dtype=torch.int32)
        clamped_o = torch.minimum(torch.clamp(wild_o, min=0), mx[None, :])
        N = A.elastic_nodes(patch[1], S)
        g = torch.Generator().manual_seed(N)
        wild_f = torch.randint(-2 ** 31, 2 ** 31, (B, N, N, 2), generator=g, dtype=torch.int64).to(torch.int32)
        wild_f[0], wild_f[1] = imax, imin
        wild_f[3] = torch.from_numpy(A.draw_elastic(1, 1, [3], patch[1], S / 8.0, S)[0])
        clamped_f = wild_f.clamp(-(1 << 22), 1 << 22)
        idx = batch_idx(B, dev)
        code = torch.arange(B, dtype=torch.int32) + 4
        good_m, good_o = matrices("defaults", B), origins(B, stored, patch)
        for m, o, f, wm, wo, wf in ((wild_m, good_o, None, clamped_m, good_o, None),
                                    (good_m, wild_o, None, good_m, clamped_o, None),
                                    (good_m, good_o, wild_f, good_m, good_o, clamped_f),
                                    (wild_m, wild_o, wild_f, clamped_m, clamped_o, clamped_f)):
            got = warp3_gather(x_all, y_all, idx, o.to(dev), code.to(dev), m.to(dev), None,
                               f.to(dev) if f is not None else None, S, tname, cpad, patch)
            w = oracle(x_all, y_all, idx, wo, code, wm, wf, S, tname, cpad, patch)
            assert torch.equal(bits(got[0]), bits(w[0])) and torch.equal(bits(got[1]), bits(w[1])), (tname, cin)


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_bad_shapes_and_missing_pointers_are_refused(cuda_dev, tname):
    """gather_check in the bindings: nothing is launched, the outputs keep their NaNs."""
    dev = cuda_dev
    dt, pre, dt_id, _ = TYPES[tname]
    op = pre + "gather_batch_warp3"
    stored, patch = SHAPES[0]
    x_all, y_all = dataset(stored, 4, 2)
    B = 4
    idx = batch_idx(B, dev)
    mat = matrices("defaults", B).to(dev)
    field = fields(B, 32, 16).to(dev)
    n = B * patch[0] * patch[1] * patch[2]
    xb = torch.full((n * 4,), float("nan"), dtype=dt, device=dev)
    tb = torch.full((n * 2,), float("nan"), dtype=dt, device=dev)
    ptrs = [ptr(x_all), ptr(y_all), ptr(idx), 0, 0, ptr(mat), 0, ptr(field), ptr(xb), ptr(tb)]
    good = [B] + list(stored) + list(patch) + [4, 4, 2, 4]
    for ints, why in (([1, 1 << 16, 8, 8, 1 << 16, 2, 2, 4, 4, 2, 4], "D >= 2^16"),
                      (good[:10] + [2], "3 <= s <= 6"), (good[:10] + [7], "3 <= s <= 6"),
                      ([B] + list(stored) + [10, 32, 32, 4, 4, 2, 4], "exceeds"),        # patch > stored
                      ([B] + list(stored) + [5, 32, 16, 4, 4, 2, 4], "H == W")):
        with pytest.raises(ValueError) as e:
            C().generic(op, ptrs, ints, [], stream(), dt_id)
        assert "gather_batch_warp3" in str(e.value) and why in str(e.value)
    for missing in (0, 1, 2, 5, 8, 9):              # (5: a null matrix)
        with pytest.raises(ValueError):
            C().generic(op, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], stream(), dt_id)
    torch.cuda.synchronize()
    assert torch.isnan(xb.float()).all() and torch.isnan(tb.float()).all()
    C().generic(op, ptrs[:7] + [0] + ptrs[8:], good[:10] + [0], [], stream(), dt_id)      # (no field: s is not read)
    torch.cuda.synchronize()
    assert torch.isfinite(xb.float()).all() and torch.isfinite(tb.float()).all()


# ------------------------------------------------------------------ executors
def _backend(dev, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(batch_size=4, img_size=16, dims=3, in_channels=4, synthetic=True, no_checkpoint=True, **kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    return cfg, flat, NativeBackend(spec, flat, cfg, dev, 4)


def _resident(dev, cfg, aug, crop, stored=24, cell=8):
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.data.loader import ResidentBatch
    x, y = synthetic_brats(NALL, stored, cfg.in_channels, cfg.dims, seed=5, out_channels=cfg.out_channels)
    idx = torch.tensor([1, 4, 4, 3], dtype=torch.int64, device=dev)
    return ResidentBatch(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), idx, aug, crop, cell)


class Recorder:
    """The extension module with `generic` recording the op names it launches."""

    def __init__(self, mod):
        self._mod, self.kinds = mod, []

    def generic(self, kind, *a):
        self.kinds.append(kind)
        return self._mod.generic(kind, *a)

    def __getattr__(self, name):
        return getattr(self._mod, name)


@pytest.mark.parametrize("kw", [dict(out_channels=1), dict(out_channels=3), dict(out_channels=1, dtype="fp32")],
                         ids=["bf16-K1", "bf16-K3", "fp32-K1"])
def test_executor_load_indexed_with_3d_matrices(cuda_dev, kw):
    """load_indexed(aug=(code, affine, mat3[, field]), crop=...) fills the executor's input and target
    with the oracle's bits, with and without crop and field; a step on the batch runs; without a
    9-entry matrix the ops launched are the ones launched before."""
    dev = cuda_dev
    cfg, flat, be = _backend(dev, **kw)
    e = be.engine
    fp32 = kw.get("dtype") == "fp32"
    tname = "fp32" if fp32 else "bf16"
    pre = "f32_" if fp32 else ""
    T = (16, 16, 16)
    code = torch.tensor([13, 2, 7, 8], dtype=torch.int32, device=dev)
    mat = matrices("axis30", 16)[[0, 4, 8, 12]].contiguous().to(dev)
    org = torch.tensor([[0, 8, 3], [8, 0, 0], [3, 7, 8], [1, 2, 5]], dtype=torch.int32, device=dev)
    field = torch.from_numpy(A.draw_elastic(2, 9, [1, 4, 4, 3], 16, 1.0, 8)).to(dev)
    e.C = rec = Recorder(e.C)
    for stored, crop in ((24, (org, T)), (16, None)):
        for fld in (None, field):
            aug = (code, None, mat) + ((fld,) if fld is not None else ())
            rb = _resident(dev, cfg, aug, crop, stored)
            rec.kinds.clear()
            e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=rb.aug, crop=rb.crop, elastic_cell=8)
            torch.cuda.synchronize()
            assert rec.kinds == [pre + "gather_batch_warp3"]
            wx, wy = oracle(rb.x_all, rb.y_all, rb.idx, crop[0] if crop else None, code, mat, fld, 8, tname, 4, T)
            assert torch.equal(bits(e.bufs["x"].view(-1)), bits(wx.view(-1)))
            assert torch.equal(bits(e.target.view(-1)), bits(wy.view(-1)))
            assert (wx.float() == 0).any() and (wx.float() != 0).any()
            tx, ty = rb.tensors()                      # what any other backend is handed
            ox, oy = oracle32(rb.x_all, rb.y_all, rb.idx, crop[0] if crop else None, code, mat, fld, 8, T)
            assert torch.equal(tx, ox) and torch.equal(ty, oy)
            be.fwd_bwd(rb, None, seed=7)
            torch.cuda.synchronize()
            assert torch.isfinite(flat.grad).all() and flat.grad.abs().sum() > 0
    # without a 9-entry matrix: today's ops, by name
    m2 = torch.from_numpy(A.draw_spatial(1, 1, np.arange(4), "rotate")).to(dev)
    rb = _resident(dev, cfg, (code, None), (org, T), 24)
    for aug, want in (((code, None), "gather_batch_crop"), (None, "gather_batch_crop"), ((code, None, None), "gather_batch_crop"),
                      ((code, None, m2), "gather_batch_warp"), ((code, None, m2, field), "gather_batch_elastic"),
                      ((code, None, None, field), "gather_batch_elastic")):
        rec.kinds.clear()
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=aug, crop=rb.crop, elastic_cell=8)
        assert rec.kinds == [pre + want]
    rb = _resident(dev, cfg, (code, None), None, 16)
    rec.kinds.clear()
    e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(code, None))
    assert rec.kinds == [pre + "gather_batch_aug"]
    # a matrix of any other shape is refused, and the message names both
    for m in (mat[:, :8].contiguous(), mat.view(-1), mat.long(), mat[:3]):
        with pytest.raises(ValueError) as err:
            e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(code, None, m))
        assert "[4][4]" in str(err.value) and "[4][9]" in str(err.value)
    torch.cuda.synchronize()


def test_resident_feeder_uploads_the_nine_entry_rows(cuda_dev):
    """DeviceFeeder on resident data: the 3 x 3 matrices reach the device unchanged in the one upload,
    behind the codes and the origins and before the field; the lazy batch, its tensors and the
    non-lazy batch are the same batch; an executor takes it."""
    from unet_distributed_amd.data.loader import DeviceFeeder
    cfg, flat, be = _backend(cuda_dev, out_channels=1)
    idx = [3, 1, 4, 4]
    T = (16, 16, 16)
    for stored, patch, elastic in ((24, T, False), (24, T, True), (16, None, True)):
        rb0 = _resident(cuda_dev, cfg, None, None, stored)
        xs, ys = rb0.x_all.cpu().numpy(), rb0.y_all.cpu().numpy()
        f = DeviceFeeder(xs, ys, 4, cuda_dev, mode="on", patch=patch, elastic_cell=8)
        assert f.resident

        def aug(si):
            code, aff = A.draw(3, 5, si, "flip,rot90,intensity", 4, 3, 0.2)
            out = (code, aff) + ((A.draw_crop(3, 5, si, (stored,) * 3, T, "random")[0],) if patch else ())
            out += (A.draw_spatial3(3, 5, si, "rotate3d,scale3d", 30.0, 15.0, 0.25),)
            return out + ((A.draw_elastic(3, 5, si, 16, 1.0, 8),) if elastic else ())

        drawn = aug(np.array(sorted(idx)))
        code, aff = drawn[:2]
        org = drawn[2] if patch else None
        mat = drawn[3 if patch else 2]
        fld = drawn[-1] if elastic else None
        rb, none = f.get(idx, lazy=True, aug=aug)
        assert none is None and rb.idx.tolist() == sorted(idx) and len(rb.aug) == (4 if elastic else 3)
        assert rb.aug[0].cpu().tolist() == code.tolist() and torch.equal(rb.aug[1].cpu(), torch.from_numpy(aff))
        assert rb.aug[2].dtype == torch.int32 and rb.aug[2].is_contiguous() and tuple(rb.aug[2].shape) == (4, 9)
        assert torch.equal(rb.aug[2].cpu(), torch.from_numpy(mat))
        if elastic:
            assert torch.equal(rb.aug[3].cpu(), torch.from_numpy(fld))
        if patch:
            assert torch.equal(rb.crop[0].cpu(), torch.from_numpy(org)) and tuple(rb.crop[1]) == patch
        x, y = f.get(idx, aug=aug)
        tx, ty = rb.tensors()
        wx, wy = A.warp3_torch(rb0.x_all[sorted(idx)], rb0.y_all[sorted(idx)], org, T, mat, (fld, 8) if elastic else None)
        wx, wy = A.apply_torch(wx, wy, code, aff)
        assert torch.equal(x, wx) and torch.equal(y, wy) and torch.equal(tx, wx) and torch.equal(ty, wy)
        be.engine.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=rb.aug, crop=rb.crop, elastic_cell=8)
        torch.cuda.synchronize()
        got = be.engine.bufs["x"].view(wx.shape).float()
        assert (got - wx).abs().max() <= 2.0 ** -7 * wx.abs().max()         # (bf16 of the same voxels)
        assert torch.equal(be.engine.target.view(wy.shape).float(), wy)


def test_cli_trains_with_rotate3d_and_scale3d(cuda_dev, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "--dims", "3", "--synthetic_size", "24",
           "--img_size", "16", "--in_channels", "4", "--batch_size", "4", "--synthetic_train", "8", "--synthetic_test", "4",
           "--crop", "random", "--augment", "flip,rotate3d,scale3d,elastic,intensity", "--steps", "3", "--no_checkpoint",
           "--notensorboard", "--noexport", "--log_jsonl", str(tmp_path / "m.jsonl")]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout
    assert "backend native" in out, out[-3000:]
    assert ("Training augmentation: flip, rotate3d, scale3d, elastic, intensity (amplitude 0.1) (rotate +-30 deg) "
            "(out of plane +-15 deg) (scale 0.8..1.25, depth too) (elastic sigma 4 px, cell 32)") in out, out[-3000:]
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    train = [q for q in recs if q["kind"] == "train"]
    assert train and train[-1]["step"] == 3 and np.isfinite(train[-1]["loss"])
    assert train[-1]["augment"] == {"rotate_deg": [-30.0, 30.0], "rotate3d_deg": [-15.0, 15.0], "scale": [0.8, 1.25],
                                    "scale_depth": True, "elastic": {"sigma_px": 4.0, "cell": 32}}
    final = [q for q in recs if q["kind"] == "test_final"]
    assert len(final) == 1 and all(np.isfinite(final[0][k]) for k in ("loss", "dice", "sensitivity", "specificity"))

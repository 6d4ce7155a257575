"""Elastic augmentation on the GPU: the elastic batch gather (csrc/kernels/gather_resample.h, ops
gather_batch_elastic / f32_gather_batch_elastic) against the definition in plain torch --
apply_torch(elastic_torch(index_select)) cast to the storage type, bit for bit: the geometry and
the displacement are integer and every fp32 product and sum rounds on its own in both -- the
intensity affine against float64 within one rounding, field entries, matrices and origins outside
their ranges against the oracle at the clamped values, the warp and crop ops where the field is
zero, the executors' load_indexed, the feeder's upload, and one CLI run.
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
PX = 1 << 17
# name: (torch dtype, elastic op, warp op, crop op, dtype id, unit roundoff of one rounding to the type)
TYPES = {"bf16": (torch.bfloat16, "gather_batch_elastic", "gather_batch_warp", "gather_batch_crop", 0, 2.0 ** -8),
         "fp16": (torch.float16, "gather_batch_elastic", "gather_batch_warp", "gather_batch_crop", 1, 2.0 ** -11),
         "fp32": (torch.float32, "f32_gather_batch_elastic", "f32_gather_batch_warp", "f32_gather_batch_crop", 0,
                  2.0 ** -24)}
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
    """The resident fp32 dataset of one stored shape ((Hs, Ws) or (Ds, Hs, Ws)), shared by the
    tests that read it and never written (randn: no negative zeros)."""
    g = torch.Generator().manual_seed(sum(stored) * 100 + 10 * cin + K)
    x = torch.randn((NALL,) + tuple(stored) + (cin,), generator=g)
    y = (torch.rand((NALL,) + tuple(stored) + (K,), generator=g) > 0.6).float()
    return x.cuda(), y.cuda()


def batch_idx(B, dev):
    """Unsorted sample indices out of NALL with repeats."""
    idx = [3, 2, 4, 2, 0, 1, 3, 4, 1, 0, 2, 4, 3, 1, 0, 2][:B]
    return torch.tensor(idx, dtype=torch.int64, device=dev)


def origins(B, stored3, patch3):
    """int32 [B][3]: 0, the maximum, odd values and mixtures, all inside [0, S - T]."""
    mx = [s - t for s, t in zip(stored3, patch3)]
    rows = [(0, 0, 0), tuple(mx), (1, 1, 3), (mx[0], 0, mx[2]), (0, mx[1], 0), (3, 5, 7), (mx[0] - 1, mx[1] - 1, 1),
            (1, mx[1], mx[2] - 1)]
    rows = [tuple(min(max(v, 0), m) for v, m in zip(r, mx)) for r in rows]
    return torch.tensor([rows[i % len(rows)] for i in range(B)], dtype=torch.int32)


def rot(deg, z):
    t = np.radians(deg)
    c, s = int(np.rint(ONE * np.cos(t) / z)), int(np.rint(ONE * np.sin(t) / z))
    return [c, -s, s, c]


def matrices(B):
    """int32 [B][4]: the identity, the quarter turns, 45 degrees at zoom 0.7 (reads outside the
    image), 10 degrees at zoom 1.4, -170 degrees, and rows of draw_spatial."""
    rows = [A.mat_of_code(c).tolist() for c in A.ROT90_CODES] + [rot(45, 0.7), rot(10, 1.4), rot(-170, 1.0)]
    rows += A.draw_spatial(11, 3, np.arange(16), "rotate,scale", 30.0, 0.25).tolist()
    return torch.tensor(rows[:B], dtype=torch.int32)


def fields(B, side, S):
    """int32 [B][N][N][2]: draw_elastic at the largest amplitude the flags admit (S / 8 pixels),
    one sample at the clamp's extremes and one all zero."""
    f = A.draw_elastic(7, 2, np.arange(B), side, S / 8.0, S)
    f[1, ::2], f[1, 1::2] = 1 << 22, -(1 << 22)
    f[2] = 0
    return torch.from_numpy(f)


def codes(B, ncode):
    code = torch.tensor([(3 * i + 5) % ncode for i in range(B)], dtype=torch.int32)     # every code, shuffled
    assert sorted(code.tolist()) == sorted(list(range(ncode)) * (B // ncode))
    return code


def dims3(v):
    return (1,) + tuple(v) if len(v) == 2 else tuple(v)


def log2(S):
    return int(S).bit_length() - 1


def elastic_gather(x_all, y_all, idx, origin, code, mat, affine, field, S, tname, cpad, patch):
    """gather_batch_elastic / f32_gather_batch_elastic into guarded buffers; patch (H, W) or (D, H, W)."""
    dt, op, _, _, dt_id, _ = TYPES[tname]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    Ds, Hs, Ws = dims3(x_all.shape[1:-1])
    D, H, W = dims3(patch)
    assert tuple(field.shape) == (B, A.elastic_nodes(H, S), A.elastic_nodes(H, S), 2) and field.is_contiguous()
    xb = Guarded(B * D * H * W * cpad, dt, x_all.device)
    tb = Guarded(B * D * H * W * K, dt, x_all.device)
    C().generic(op, [ptr(x_all), ptr(y_all), ptr(idx), ptr(origin), ptr(code), ptr(mat), ptr(affine), ptr(field),
                     ptr(xb.out), ptr(tb.out)], [B, Ds, Hs, Ws, D, H, W, cin, cpad, K, log2(S)], [], stream(), dt_id)
    torch.cuda.synchronize()
    xb.check()
    tb.check()
    return xb.out.view((B,) + tuple(patch) + (cpad,)), tb.out.view((B,) + tuple(patch) + (K,))


def other_gather(which, x_all, y_all, idx, origin, code, mat, tname, cpad, patch):
    """gather_batch_warp (which = 2) or gather_batch_crop (3) with the same arguments."""
    dt, dt_id = TYPES[tname][0], TYPES[tname][4]
    B, cin, K = idx.numel(), x_all.shape[-1], y_all.shape[-1]
    Ds, Hs, Ws = dims3(x_all.shape[1:-1])
    D, H, W = dims3(patch)
    xb = torch.empty(B * D * H * W * cpad, dtype=dt, device=x_all.device)
    tb = torch.empty(B * D * H * W * K, dtype=dt, device=x_all.device)
    ptrs = [ptr(x_all), ptr(y_all), ptr(idx), ptr(origin), ptr(code)] + ([ptr(mat)] if which == 2 else []) + \
        [0, ptr(xb), ptr(tb)]
    C().generic(TYPES[tname][which], ptrs, [B, Ds, Hs, Ws, D, H, W, cin, cpad, K], [], stream(), dt_id)
    torch.cuda.synchronize()
    return xb.view((B,) + tuple(patch) + (cpad,)), tb.view((B,) + tuple(patch) + (K,))


def oracle32(x_all, y_all, idx, origin, code, mat, field, S, patch):
    """apply_torch(elastic_torch(plain index_select)) in fp32, no affine."""
    x, y = A.elastic_torch(x_all.index_select(0, idx), y_all.index_select(0, idx), origin, dims3(patch), mat, field, S)
    return A.apply_torch(x, y, code if code is not None else np.zeros(idx.numel(), np.int32))


def oracle(x_all, y_all, idx, origin, code, mat, field, S, tname, cpad, patch):
    """... cast to the type, zero pad channels."""
    dt = TYPES[tname][0]
    x, y = oracle32(x_all, y_all, idx, origin, code, mat, field, S, patch)
    xb = torch.zeros(x.shape[:-1] + (cpad,), dtype=dt, device=x.device)
    xb[..., :x.shape[-1]] = x.to(dt)
    return xb, y.to(dt)


def cpad_of(tname, cin):
    return cin if tname == "fp32" else (4 if cin <= 4 else 8 if cin <= 8 else cin)


def check_elastic(dev, tname, stored, patch, S, cin, K, B=16, null_origin=False, null_mat=False):
    cpad = cpad_of(tname, cin)
    x_all, y_all = dataset(tuple(stored), cin, K)
    idx = batch_idx(B, dev)
    code = codes(B, 8 if len(stored) == 2 else 16)
    mat = None if null_mat else matrices(B)
    dmat = None if null_mat else mat.to(dev)
    field = fields(B, patch[-1], S)
    org = None if null_origin else origins(B, dims3(stored), dims3(patch))
    dorg = None if null_origin else org.to(dev)
    wx, wt = oracle(x_all, y_all, idx, org, code, mat, field, S, tname, cpad, patch)
    gx, gt = elastic_gather(x_all, y_all, idx, dorg, code.to(dev), dmat, None, field.to(dev), S, tname, cpad, patch)
    assert torch.equal(bits(gx), bits(wx)), (tname, stored, patch, S, cin, cpad, K, "image")
    assert torch.equal(bits(gt), bits(wt)), (tname, stored, patch, S, cin, cpad, K, "target")
    if not null_mat:
        assert (gx[4].float() == 0).any() and (gx[4].float() != 0).any()    # 45 degrees at zoom 0.7 leaves the image
    if cpad > cin:
        assert (gx[..., cin:] == 0).all()
    # the field is not a no-op: sample 2's is zero, the others' are not
    zx, _ = oracle(x_all, y_all, idx, org, code, mat, torch.zeros_like(field), S, tname, cpad, patch)
    assert torch.equal(bits(zx[2]), bits(wx[2])) and not torch.equal(bits(zx[0]), bits(wx[0]))
    # two runs give the same bits
    hx, ht = elastic_gather(x_all, y_all, idx, dorg, code.to(dev), dmat, None, field.to(dev), S, tname, cpad, patch)
    assert torch.equal(bits(gx), bits(hx)) and torch.equal(bits(gt), bits(ht))


# Cin 4 with K 1 and 3: the 16-byte tap loads; Cin 1 and 3: padded to 4; Cin 5: Cpad 8; Cin 12: one lane per pixel
CHANNELS = [(4, 1), (4, 3), (1, 1), (3, 2), (5, 1), (12, 2)]


@pytest.mark.parametrize("stored,T,S", [((40, 48), 32, 8), ((56, 72), 40, 16), ((40, 48), 32, 64)],
                         ids=["several-cells", "ragged-last-cell", "one-cell-larger-than-the-patch"])
@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_2d(cuda_dev, tname, stored, T, S):
    """Patch 32 of 40 x 48 with S = 8: a tile stages 6 of its 7 x 7 nodes per axis; patch 40 of
    56 x 72 with S = 16: two tiles per axis, a ragged last cell, N = 5; patch 32 with S = 64: one
    cell larger than the patch, N = 3.  All 8 codes, mixed matrices."""
    assert A.elastic_nodes(T, S) == {8: 6, 16: 5, 64: 3}[S]
    for cin, K in CHANNELS:
        check_elastic(cuda_dev, tname, stored, (T, T), S, cin, K)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_2d_null_matrix_and_null_origin(cuda_dev, tname):
    """--augment elastic without rotate / scale (a null `mat` is the identity) and without --crop
    (a null origin on samples of the patch size: every tap outside the patch is outside the image)."""
    for cin, K in ((4, 1), (3, 2), (12, 1)):
        check_elastic(cuda_dev, tname, (40, 48), (32, 32), 32, cin, K, null_mat=True)
        check_elastic(cuda_dev, tname, (32, 32), (32, 32), 32, cin, K, null_origin=True)
        check_elastic(cuda_dev, tname, (32, 32), (32, 32), 16, cin, K, null_origin=True, null_mat=True)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_3d_all_sixteen_codes(cuda_dev, tname):
    """Every slice through the sample's matrix and field, FD picking the slice."""
    for cin, K in ((4, 2), (5, 1), (12, 1)):
        check_elastic(cuda_dev, tname, (5, 48, 56), (3, 40, 40), 16, cin, K)


@pytest.mark.parametrize("tname", list(TYPES))
def test_kernel_intensity_within_one_rounding(cuda_dev, tname):
    """|out - r| <= 2 u |r| + 2^-22 (|scale v| + |shift|) + 2^-24 with r = scale v + shift in
    float64 and v the oracle's fp32 interpolation: one rounding to the storage type (unit
    roundoff u) with a factor-2 margin, plus the fp32 evaluation of the fma -- the bound of the
    warp gather's test.  The target is the geometry's alone."""
    dev = cuda_dev
    u = TYPES[tname][5]
    worst = 0.0
    for stored, patch, S, cin, K in (((40, 48), (32, 32), 8, 4, 3), ((40, 48), (32, 32), 32, 1, 1),
                                     ((40, 48), (32, 32), 16, 12, 1), ((5, 48, 56), (3, 40, 40), 16, 4, 2)):
        B = 16
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx, code, mat = batch_idx(B, dev), codes(B, 8 if len(stored) == 2 else 16), matrices(B)
        field = fields(B, patch[-1], S)
        org = origins(B, dims3(stored), dims3(patch))
        g = torch.Generator().manual_seed(cin + K)
        a = 0.25
        aff = torch.stack([1 - a + 2 * a * torch.rand(B, cin, generator=g),
                           -a + 2 * a * torch.rand(B, cin, generator=g)], dim=-1).contiguous()
        args = (x_all, y_all, idx, org.to(dev), code.to(dev), mat.to(dev))
        gx, gt = elastic_gather(*args, aff.to(dev), field.to(dev), S, tname, cpad, patch)
        _, t0 = elastic_gather(*args, None, field.to(dev), S, tname, cpad, patch)
        assert torch.equal(bits(gt), bits(t0))
        xg, _ = oracle32(x_all, y_all, idx, org, code, mat, field, S, patch)
        sh = (B,) + (1,) * (xg.dim() - 2) + (cin,)
        s, t = aff[..., 0].to(dev).double().view(sh), aff[..., 1].to(dev).double().view(sh)
        r = s * xg.double() + t
        bound = 2 * u * r.abs() + 2.0 ** -22 * ((s * xg.double()).abs() + t.abs()) + 2.0 ** -24
        err = (gx[..., :cin].double() - r).abs()
        worst = max(worst, float((err / bound).max()))
        print("intensity", tname, (stored, patch, S, cin, K), "max err / bound", float((err / bound).max()))
        assert (err <= bound).all(), (tname, stored, cin, K)
        if cpad > cin:
            assert (gx[..., cin:] == 0).all()
    assert worst > 0


@pytest.mark.parametrize("tname", list(TYPES))
def test_a_zero_field_is_the_warp_gather_and_with_a_null_matrix_the_crop_gather(cuda_dev, tname):
    dev = cuda_dev
    for stored, patch, S, cin, K in (((40, 48), (32, 32), 8, 4, 3), ((40, 48), (32, 32), 64, 12, 1),
                                     ((5, 48, 56), (3, 40, 40), 16, 4, 1)):
        B = 16
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, K)
        idx = batch_idx(B, dev)
        org = origins(B, dims3(stored), dims3(patch)).to(dev)
        code = codes(B, 8 if len(stored) == 2 else 16).to(dev)
        mat = matrices(B).to(dev)
        zero = torch.zeros_like(fields(B, patch[-1], S)).to(dev)
        a = elastic_gather(x_all, y_all, idx, org, code, mat, None, zero, S, tname, cpad, patch)
        b = other_gather(2, x_all, y_all, idx, org, code, mat, tname, cpad, patch)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), (tname, stored, cin)
        a = elastic_gather(x_all, y_all, idx, org, code, None, None, zero, S, tname, cpad, patch)
        b = other_gather(3, x_all, y_all, idx, org, code, None, tname, cpad, patch)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), (tname, stored, cin)
        n = elastic_gather(x_all, y_all, idx, org, None, mat, None, zero, S, tname, cpad, patch)     # null code == code 0
        z = elastic_gather(x_all, y_all, idx, org, torch.zeros_like(code), mat, None, zero, S, tname, cpad, patch)
        assert torch.equal(bits(n[0]), bits(z[0])) and torch.equal(bits(n[1]), bits(z[1]))


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_fields_matrices_and_origins_outside_their_ranges_are_clamped(cuda_dev, tname):
    """Field entries beyond +-2^22, matrix entries beyond +-2^18 and origins outside the sample
    (device data no launch can validate) read through the clamped values; every address stays
    inside the slice by the kernel's own clamps: tiled and per-pixel kernels, 2D and 3D."""
    dev = cuda_dev
    for stored, patch, S, cin in (((40, 48), (32, 32), 8, 4), ((40, 48), (32, 32), 32, 12),
                                  ((5, 48, 56), (3, 40, 40), 16, 4)):
        cpad = cpad_of(tname, cin)
        x_all, y_all = dataset(stored, cin, 2)
        B = 8
        Sd, T = dims3(stored), dims3(patch)
        big = 1 << 20
        wild_m = torch.tensor([[big, -big, big, -big], [-big, big, big, big], [big, 0, 0, -big], [ONE, -big, big, ONE],
                               [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31], [-2 ** 31, 0, 3, 2 ** 31 - 1],
                               [(1 << 18) + 1, 0, 0, -(1 << 18) - 1], rot(30, 1.0)], dtype=torch.int32)
        clamped_m = wild_m.clamp(-(1 << 18), 1 << 18)
        wild_o = torch.tensor([(-1, -1, -1), (0, -7, 1000), (5000, 9, -3), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1),
                               (-2 ** 31, -2 ** 31, -2 ** 31), (1, Sd[1] - T[1] + 1, 3), (0, 2, Sd[2] - T[2] + 1),
                               (Sd[0] - T[0] + 1, 0, 0)], dtype=torch.int32)
        mx = torch.tensor([s - t for s, t in zip(Sd, T)], dtype=torch.int32)
        clamped_o = torch.minimum(torch.clamp(wild_o, min=0), mx[None, :])
        N = A.elastic_nodes(T[1], S)
        g = torch.Generator().manual_seed(N)
        wild_f = torch.randint(-2 ** 31, 2 ** 31, (B, N, N, 2), generator=g, dtype=torch.int64).to(torch.int32)
        wild_f[0] = 2 ** 31 - 1
        wild_f[1] = -2 ** 31
        wild_f[2, 0, 0, 0], wild_f[2, 0, 0, 1] = (1 << 22) + 1, -(1 << 22) - 1
        wild_f[3] = torch.from_numpy(A.draw_elastic(1, 1, [3], T[1], S / 8.0, S)[0])
        clamped_f = wild_f.clamp(-(1 << 22), 1 << 22)
        assert not torch.equal(wild_f, clamped_f)
        idx = batch_idx(B, dev)
        code = torch.arange(B, dtype=torch.int32)
        eye = torch.tensor([[ONE, 0, 0, ONE]] * B, dtype=torch.int32)
        good_o = origins(B, Sd, T)
        for m, o, f, wm, wo, wf in ((eye, good_o, wild_f, eye, good_o, clamped_f),
                                    (wild_m, wild_o, clamped_f, clamped_m, clamped_o, clamped_f),
                                    (wild_m, wild_o, wild_f, clamped_m, clamped_o, clamped_f)):
            got = elastic_gather(x_all, y_all, idx, o.to(dev), code.to(dev), m.to(dev), None, f.to(dev), S, tname, cpad,
                                 patch)
            w = oracle(x_all, y_all, idx, wo, code, wm, wf, S, tname, cpad, patch)
            assert torch.equal(bits(got[0]), bits(w[0])) and torch.equal(bits(got[1]), bits(w[1])), (tname, stored, cin)


@pytest.mark.parametrize("tname", ["bf16", "fp32"])
def test_bad_shapes_and_missing_pointers_are_refused(cuda_dev, tname):
    """gather_check in the bindings: nothing is launched, the outputs keep their NaNs."""
    dev = cuda_dev
    dt, op, _, _, dt_id, _ = TYPES[tname]
    x_all, y_all = dataset((40, 48), 4, 2)
    B = 4
    idx = batch_idx(B, dev)
    mat = matrices(B).to(dev)
    field = fields(B, 32, 16).to(dev)
    xb = torch.full((B * 32 * 32 * 4,), float("nan"), dtype=dt, device=dev)
    tb = torch.full((B * 32 * 32 * 2,), float("nan"), dtype=dt, device=dev)
    ptrs = [ptr(x_all), ptr(y_all), ptr(idx), 0, 0, ptr(mat), 0, ptr(field), ptr(xb), ptr(tb)]
    good = [B, 1, 40, 48, 1, 32, 32, 4, 4, 2, 4]
    for ints in ([B, 1, 40, 48, 1, 48, 48, 4, 4, 2, 4],            # patch > stored
                 [B, 1, 40, 48, 2, 32, 32, 4, 4, 2, 4],
                 [B, 1, 40, 48, 1, 32, 32, 4, 4, 5, 4],            # K > 4
                 [B, 1, 40, 48, 1, 32, 16, 4, 4, 2, 4],            # H != W
                 [B, 1, 40, 48, 1, 32, 32, 4, 4, 2, 2],            # 3 <= s <= 6
                 [B, 1, 40, 48, 1, 32, 32, 4, 4, 2, 7],
                 [B, 1, 40, 48, 1, 32, 32, 4, 4, 2, 16]):
        with pytest.raises(ValueError) as e:
            C().generic(op, ptrs, ints, [], stream(), dt_id)
        assert "gather_batch_elastic" in str(e.value)
    for missing in (0, 1, 2, 7, 8, 9):
        with pytest.raises(ValueError):
            C().generic(op, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], stream(), dt_id)
    with pytest.raises(ValueError):
        C().generic(op, ptrs[:9], good, [], stream(), dt_id)
    with pytest.raises(ValueError):
        C().generic(op, ptrs, good[:10], [], stream(), dt_id)
    torch.cuda.synchronize()
    assert torch.isnan(xb.float()).all() and torch.isnan(tb.float()).all()
    C().generic(op, ptrs, good, [], stream(), dt_id)            # (and the good call runs)
    torch.cuda.synchronize()
    assert torch.isfinite(xb.float()).all() and torch.isfinite(tb.float()).all()


# ------------------------------------------------------------------ executors
def _backend(dev, **kw):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(batch_size=4, img_size=32, in_channels=4, synthetic=True, no_checkpoint=True, **kw)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    return cfg, flat, NativeBackend(spec, flat, cfg, dev, 4)


def _resident(dev, cfg, aug, crop, stored=48, cell=32):
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.data.loader import ResidentBatch
    x, y = synthetic_brats(NALL, stored, cfg.in_channels, cfg.dims, seed=5, out_channels=cfg.out_channels)
    idx = torch.tensor([1, 4, 4, 3], dtype=torch.int64, device=dev)
    return ResidentBatch(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), idx, aug, crop, elastic_cell=cell)


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
def test_executor_load_indexed_with_a_field(cuda_dev, kw):
    """load_indexed(aug=(code, affine, mat or None, field), crop=...) launches exactly the elastic op
    and fills the executor's input and target with the oracle's bits (no affine) or within one
    rounding of it (affine), with and without crop and matrices; a step on the batch runs; an
    `aug` of three or two items launches the ops launched before."""
    dev = cuda_dev
    cfg, flat, be = _backend(dev, **kw)
    e = be.engine
    fp32 = kw.get("dtype") == "fp32"
    tname = "fp32" if fp32 else "bf16"
    pre = "f32_" if fp32 else ""
    S = 16
    code = torch.tensor([5, 2, 7, 0], dtype=torch.int32, device=dev)
    mat = torch.tensor([rot(45, 0.7), rot(-20, 1.2), A.mat_of_code(3).tolist(), rot(170, 1.0)], dtype=torch.int32,
                       device=dev)
    field = torch.from_numpy(A.draw_elastic(2, 9, [1, 4, 4, 3], 32, 2.0, S)).to(dev)
    org = torch.tensor([[0, 16, 3], [0, 0, 0], [0, 7, 16], [0, 9, 5]], dtype=torch.int32, device=dev)
    aff = torch.tensor([[[1.1, -0.05]] * 4, [[0.9, 0.1]] * 4, [[1.0, 0.0]] * 4, [[1.2, 0.2]] * 4], device=dev)
    e.C = rec = Recorder(e.C)
    for stored, crop, m in ((48, (org, (1, 32, 32)), mat), (32, None, None), (48, (org, (1, 32, 32)), None)):
        rb = _resident(dev, cfg, (code, None, m, field), crop, stored, S)
        rec.kinds.clear()
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=rb.aug, crop=rb.crop, elastic_cell=S)
        torch.cuda.synchronize()
        assert rec.kinds == [pre + "gather_batch_elastic"]
        o = crop[0] if crop else None
        wx, wy = oracle(rb.x_all, rb.y_all, rb.idx, o, code, m, field, S, tname, 4, (32, 32))
        assert torch.equal(bits(e.bufs["x"].view(-1)), bits(wx.view(-1)))
        assert torch.equal(bits(e.target.view(-1)), bits(wy.view(-1)))
        tx, ty = rb.tensors()                      # what any other backend is handed
        assert torch.equal(tx, oracle32(rb.x_all, rb.y_all, rb.idx, o, code, m, field, S, (32, 32))[0])
        # with the affine: one rounding of scale v + shift
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(code, aff, m, field), crop=rb.crop, elastic_cell=S)
        torch.cuda.synchronize()
        u = TYPES[tname][5]
        r = tx.double() * aff[:, None, None, :, 0].double() + aff[:, None, None, :, 1].double()
        err = (e.bufs["x"].view(tx.shape).double() - r).abs()
        assert (err <= 2 * u * r.abs() + 2.0 ** -22 * (r.abs() + 1) + 2.0 ** -24).all()
        assert torch.equal(bits(e.target.view(-1)), bits(wy.view(-1)))
        # a step on the batch runs, through the backend's own dispatch on the batch
        rec.kinds.clear()
        be.fwd_bwd(rb, None, seed=7)
        torch.cuda.synchronize()
        assert rec.kinds[0] == pre + "gather_batch_elastic" and not any("gather" in k for k in rec.kinds[1:])
        assert torch.isfinite(flat.grad).all() and flat.grad.abs().sum() > 0
    # three and two items: today's ops, by name
    rb = _resident(dev, cfg, (code, None), (org, (1, 32, 32)), 48)
    for aug, crop, want in (((code, None, mat), rb.crop, "gather_batch_warp"), ((code, None), rb.crop, "gather_batch_crop"),
                            (None, rb.crop, "gather_batch_crop"), ((code, None, None), rb.crop, "gather_batch_crop")):
        rec.kinds.clear()
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=aug, crop=crop)
        assert rec.kinds == [pre + want]
    rb = _resident(dev, cfg, (code, None), None, 32)
    for aug, want in (((code, None, mat), "gather_batch_warp"), ((code, None), "gather_batch_aug")):
        rec.kinds.clear()
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=aug)
        assert rec.kinds == [pre + want]
    torch.cuda.synchronize()


def test_gather_elastic_args_refuses_wrong_tensors(cuda_dev):
    cfg, flat, be = _backend(cuda_dev, out_channels=1)
    e = be.engine
    org = torch.zeros(4, 3, dtype=torch.int32, device=cuda_dev)
    field = torch.zeros(4, 3, 3, 2, dtype=torch.int32, device=cuda_dev)         # patch 32 at cell 32: N = 3
    rb = _resident(cuda_dev, cfg, None, None)
    crop = (org, (1, 32, 32))
    e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(None, None, None, field), crop=crop)
    for f in (field.long(), field[:3], field.cpu(), field[:, :2], field.transpose(1, 2), field.view(-1), None):
        with pytest.raises(ValueError):
            e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(None, None, None, f), crop=crop)
    with pytest.raises(ValueError):                 # the field of another cell size: N = 6 at cell 8
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(None, None, None, field), crop=crop, elastic_cell=8)
    with pytest.raises(ValueError):
        e.load_indexed(rb.x_all, rb.y_all, rb.idx, aug=(None, None, None, field), crop=crop, elastic_cell=24)
    small = _resident(cuda_dev, cfg, None, None, stored=16)
    with pytest.raises(ValueError):                 # no crop: the stored sample must hold the input
        e.load_indexed(small.x_all, small.y_all, small.idx, aug=(None, None, None, field))
    torch.cuda.synchronize()


def test_resident_feeder_uploads_the_field_behind_the_matrices(cuda_dev):
    """DeviceFeeder on resident data: the field is drawn for the sorted indices and reaches the
    device unchanged at the end of the one upload, behind the codes, the origins (with a patch)
    and the matrices (with rotate / scale), whose views are what they are without it; the lazy
    batch, its tensors and the non-lazy batch are the same batch; an executor takes it."""
    from unet_distributed_amd.data.loader import DeviceFeeder
    cfg, flat, be = _backend(cuda_dev, out_channels=1)
    idx = [3, 1, 4, 4]
    S = 8
    for stored, patch, spatial in ((48, (1, 32, 32), True), (32, None, True), (48, (1, 32, 32), False), (32, None, False)):
        rb0 = _resident(cuda_dev, cfg, None, None, stored)
        xs, ys = rb0.x_all.cpu().numpy(), rb0.y_all.cpu().numpy()
        f = DeviceFeeder(xs, ys, 4, cuda_dev, mode="on", patch=patch, elastic_cell=S)
        assert f.resident

        def aug(si, elastic=True):
            code, aff = A.draw(3, 5, si, "flip,rot90,intensity", 4, 2, 0.2)
            out = (code, aff) + ((A.draw_crop(3, 5, si, (1, 48, 48), (1, 32, 32), "random")[0],) if patch else ())
            mat = A.draw_spatial(3, 5, si, "rotate,scale", 30.0, 0.25) if spatial else None
            if elastic:
                return out + (mat, A.draw_elastic(3, 5, si, 32, 1.0, S))
            return out + ((mat,) if spatial else ())

        drawn = aug(np.array(sorted(idx)))
        code, aff, mat, field = drawn[0], drawn[1], drawn[-2], drawn[-1]
        org = drawn[2] if patch is not None else None
        rb, none = f.get(idx, lazy=True, aug=aug)
        assert none is None and rb.idx.tolist() == sorted(idx) and len(rb.aug) == 4 and rb.elastic_cell == S
        assert rb.aug[0].cpu().tolist() == code.tolist() and torch.equal(rb.aug[1].cpu(), torch.from_numpy(aff))
        assert (rb.aug[2] is None) if not spatial else torch.equal(rb.aug[2].cpu(), torch.from_numpy(mat))
        assert rb.aug[3].dtype == torch.int32 and rb.aug[3].is_contiguous() and tuple(rb.aug[3].shape) == (4, 6, 6, 2)
        assert torch.equal(rb.aug[3].cpu(), torch.from_numpy(field))
        if patch is not None:
            assert torch.equal(rb.crop[0].cpu(), torch.from_numpy(org)) and tuple(rb.crop[1]) == patch
        else:
            assert rb.crop is None
        # the field rides at the end: the other views sit where they sit without it
        old, _ = f.get(idx, lazy=True, aug=lambda si: aug(si, False))
        assert len(old.aug) == (3 if spatial else 2)
        base = rb.idx.data_ptr()
        for a, b in zip(rb.aug[:len(old.aug)] + ((rb.crop[0],) if patch else ()),
                        old.aug + ((old.crop[0],) if patch else ())):
            assert a.data_ptr() - base == b.data_ptr() - old.idx.data_ptr() and torch.equal(a, b)
        assert rb.aug[3].data_ptr() > max(t.data_ptr() for t in rb.aug[:3] if t is not None)
        x, y = f.get(idx, aug=aug)
        tx, ty = rb.tensors()
        wx, wy = A.elastic_torch(rb0.x_all[sorted(idx)], rb0.y_all[sorted(idx)], org, (1, 32, 32), mat, field, S)
        wx, wy = A.apply_torch(wx, wy, code, aff)
        assert torch.equal(x, wx) and torch.equal(y, wy) and torch.equal(tx, wx) and torch.equal(ty, wy)
        be.fwd_bwd(rb, None, seed=3)                # (the backend's dispatch: the batch's own cell size)
        torch.cuda.synchronize()
        got = be.engine.bufs["x"].view(wx.shape).float()
        assert (got - wx).abs().max() <= 2.0 ** -7 * wx.abs().max()         # (bf16 of the same pixels)
        assert torch.equal(be.engine.target.view(wy.shape).float(), wy)


def test_cli_trains_with_elastic(cuda_dev, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "--synthetic_size", "48", "--img_size", "32",
           "--in_channels", "4", "--batch_size", "8", "--synthetic_train", "16", "--synthetic_test", "8",
           "--crop", "foreground", "--augment", "flip,rot90,rotate,scale,elastic,intensity", "--augment_elastic_cell",
           "16", "--augment_elastic", "2", "--steps", "4", "--no_checkpoint", "--notensorboard", "--noexport",
           "--log_jsonl", str(tmp_path / "m.jsonl")]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout
    assert "backend native" in out, out[-3000:]
    assert ("Training augmentation: flip, rot90, rotate, scale, elastic, intensity (amplitude 0.1) (rotate +-30 deg) "
            "(scale 0.8..1.25) (elastic sigma 2 px, cell 16)") in out, out[-3000:]
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    train = [q for q in recs if q["kind"] == "train"]
    assert train and train[-1]["step"] == 4 and np.isfinite(train[-1]["loss"])
    assert train[-1]["augment"] == {"rotate_deg": [-30.0, 30.0], "scale": [0.8, 1.25],
                                    "elastic": {"sigma_px": 2.0, "cell": 16}}
    final = [q for q in recs if q["kind"] == "test_final"]
    assert len(final) == 1 and all(np.isfinite(final[0][k]) for k in ("loss", "dice", "sensitivity", "specificity"))

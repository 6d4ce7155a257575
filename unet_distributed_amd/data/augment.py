"""Training-time augmentation: random flips, 90-degree rotations and a per-channel
brightness / contrast jitter, as per-sample parameters the batch gather applies.

A sample's transform is a 4-bit code plus an optional per-input-channel affine:

* bit 0 ``FW`` flip W, bit 1 ``FH`` flip H, bit 2 ``T`` swap H and W (square images),
  bit 3 ``FD`` flip D (3D only).  Output pixel ``(d, h, w)`` reads source pixel
  ``d' = FD ? D-1-d : d``, ``(h', w') = T ? (w, h) : (h, w)``, then ``h' = FH ? H-1-h' : h'``
  and ``w' = FW ? W-1-w' : w'`` -- image and every target channel alike.
* ``x' = scale * x + shift`` per (sample, input channel), image only.

:func:`draw` is a counter-based hash of ``(seed, step, dataset sample index)``: a
sample's parameters do not depend on the rank, the world size or its place in the
batch, so data-parallel runs of any width see one augmented global batch and a resumed
run repeats the run it resumes.  :func:`apply_torch` is the transform in plain torch
(the ATen backend, streamed data, and the oracle of the HIP kernel
``csrc/kernels/gather.h``, which applies the same parameters inside the resident
batch gather).

``--crop`` adds a patch origin per sample: :func:`draw_crop` draws it from hash words of its
own (the codes and affines above do not change), :func:`crop_torch` is the crop in plain
torch, and the whole transform is ``apply_torch(*crop_torch(x, y, origin, patch), code,
affine)`` -- the oracle of ``csrc/kernels/gather.h``.

``--augment rotate,scale`` adds a 2 x 2 matrix per sample in Q16, rotation by any angle and
isotropic zoom in the (H, W) plane: :func:`draw_spatial` draws it from hash words of its own,
:func:`warp_torch` resamples the patch through it straight from the stored sample (bilinear
image, nearest target, zero outside the image) in integer coordinates, and the whole transform
is ``apply_torch(*warp_torch(x, y, origin, patch, mat), code, affine)`` -- the oracle of
``csrc/kernels/gather_resample.h``.

``--augment elastic`` adds a smooth random deformation: :func:`draw_elastic` draws a lattice of
control-node displacements per sample (``--augment_elastic`` pixels of standard deviation, cells
of ``--augment_elastic_cell`` patch pixels) from hash words of its own, :func:`elastic_disp`
evaluates the integer quadratic B-spline through them at every patch pixel, and
:func:`elastic_torch` is warp_torch with that displacement added to its source coordinates (the
matrix is the identity without rotate / scale).  The whole transform is
``apply_torch(*elastic_torch(x, y, origin, patch, mat, field, S), code, affine)`` -- the oracle
of ``csrc/kernels/gather_resample.h``.  The order stays crop, resample, flip / quarter turns,
jitter.

``--augment rotate3d,scale3d`` (``--dims 3``) replaces the 2 x 2 matrix by a 3 x 3 one over
``(d, h, w)``: :func:`draw_spatial3` draws the in-plane angle and the zoom from draw_spatial's own
words and two out-of-plane angles (``--augment_rotate3d`` degrees) from words of their own, and
:func:`warp3_torch` resamples the patch trilinearly through it (nearest target, zero outside the
stored volume), with the elastic displacement along ``(h, w)`` when a field is given.  The whole
transform is ``apply_torch(*warp3_torch(x, y, origin, patch, mat3, disp), code, affine)`` -- the
oracle of ``gather_batch_warp3`` in ``csrc/kernels/gather_resample.h``.
"""

from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from ..config import SPATIAL3_NAMES, SPATIAL_NAMES, parse_augment, parse_crop, parse_tta

FW, FH, T, FD = 1, 2, 4, 8
# np.rot90(m, k) of the (H, W) plane for k = 0..3 as codes
ROT90_CODES = (0, T | FW, FH | FW, T | FH)

_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


def _mix(z: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _hash(seed: int, step: int, idx: np.ndarray, lanes: int, first: int = 1) -> np.ndarray:
    """uint64 [n][lanes]: independent words per (seed, step, sample index, lane); the lanes are
    numbered first .. first + lanes - 1."""
    with np.errstate(over="ignore"):
        head = _mix(np.array([(int(seed) * _GOLD + 0x632BE59BD9B4E019) & _M64], dtype=np.uint64))
        head = _mix(head ^ np.uint64((int(step) * _GOLD) & _M64))
        h = _mix(head ^ (idx.astype(np.int64).view(np.uint64) * np.uint64(0xD6E8FEB86659FD93)))
        lane = (np.arange(first, first + lanes, dtype=np.uint64) * np.uint64(_GOLD))[None, :]
        return _mix(h[:, None] + lane)


def _unit(h: np.ndarray) -> np.ndarray:
    """uint64 -> float64 in [0, 1)."""
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def _f32_within(v: np.ndarray, lo: float, hi: float) -> np.ndarray:
    """float64 in [lo, hi] -> float32 still in [lo, hi] (the rounding may step outside)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if float(lo32) < lo:
        lo32 = np.nextafter(lo32, np.float32(np.inf))
    if float(hi32) > hi:
        hi32 = np.nextafter(hi32, np.float32(-np.inf))
    return np.clip(v.astype(np.float32), lo32, hi32)


def draw(seed: int, step: int, sample_idx, spec, cin: int, dims: int,
         intensity: float = 0.1) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(code int32 [n], affine float32 [n][cin][2] = {scale, shift} or None) of the dataset
    samples `sample_idx` at global step `step`.  `spec`: the --augment string or its parsed
    names; `intensity`: the jitter amplitude a (scale in [1-a, 1+a], shift in [-a, a])."""
    names = parse_augment(spec) if isinstance(spec, str) else tuple(spec)
    idx = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    h = _hash(seed, step, idx, 1 + 2 * cin)
    r = (h[:, 0] >> np.uint64(40)).astype(np.int64)
    flip, rot = "flip" in names, "rot90" in names
    if flip and rot:
        code = r & (15 if dims == 3 else 7)
    elif flip:
        code = r & ((FW | FH | FD) if dims == 3 else (FW | FH))
    elif rot:
        code = np.asarray(ROT90_CODES, dtype=np.int64)[r & 3]
    else:
        code = np.zeros_like(r)
    affine = None
    if "intensity" in names:
        a = float(intensity)
        u = _unit(h[:, 1:]).reshape(len(idx), cin, 2)
        affine = np.empty((len(idx), cin, 2), dtype=np.float32)
        affine[..., 0] = _f32_within(1.0 - a + 2.0 * a * u[..., 0], 1.0 - a, 1.0 + a)
        affine[..., 1] = _f32_within(-a + 2.0 * a * u[..., 1], -a, a)
    return code.astype(np.int32), affine


# first hash lane of draw_crop's words: past every lane `draw` can use (1 + 2 cin of them), so a
# sample's codes and affines are the same with and without --crop
_CROP_LANE = 1 << 16


def _dims3(v) -> Tuple[int, int, int]:
    v = tuple(int(a) for a in v)
    if len(v) == 2:
        v = (1,) + v
    if len(v) != 3 or min(v) < 1:
        raise ValueError("spatial size: (D, H, W) or (H, W), all >= 1, got %r" % (v,))
    return v


def draw_crop(seed: int, step: int, sample_idx, stored, patch, mode: str, p_fg: float = 0.0,
              table=None) -> Tuple[np.ndarray, np.ndarray]:
    """(origin int32 [n][3] = (d, h, w), used_fg bool [n]) of the training patches of the
    dataset samples `sample_idx` at global step `step`: `patch` = (D, H, W) (or (H, W)) voxels of
    the `stored` = (Ds, Hs, Ws) sample.  The same counter hash as :func:`draw` with words of its
    own: an origin depends on (seed, step, dataset sample index) alone.

    `random`: o_a = floor(u_a (S_a - T_a + 1)) per axis.  `foreground`: with probability `p_fg`,
    and only for a sample with foreground, entry floor(u min(cnt, R)) of its row of `table` =
    (fg [N][R], cnt [N]) (datasets.foreground_table) is decoded to a voxel c and
    o_a = min(max(c_a - T_a // 2, 0), S_a - T_a), so the patch holds c; else the uniform rule."""
    S, T = np.array(_dims3(stored), dtype=np.int64), np.array(_dims3(patch), dtype=np.int64)
    if mode not in ("random", "foreground"):
        raise ValueError("draw_crop: mode random or foreground, got %r" % (mode,))
    if (T > S).any():
        raise ValueError("draw_crop: patch %r exceeds the stored sample %r" % (tuple(T), tuple(S)))
    idx = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    u = _unit(_hash(seed, step, idx, 5, first=_CROP_LANE))
    span = S - T + 1
    origin = np.minimum(np.floor(u[:, 2:5] * span[None, :]).astype(np.int64), (S - T)[None, :])
    used = np.zeros(len(idx), dtype=bool)
    if mode == "foreground":
        if table is None:
            raise ValueError("draw_crop: the foreground mode needs the foreground table")
        fg, cnt = table
        n = np.minimum(np.asarray(cnt)[idx].astype(np.int64), fg.shape[1])
        used = (u[:, 0] < float(p_fg)) & (n > 0)
        j = np.minimum(np.floor(u[:, 1] * n).astype(np.int64), np.maximum(n - 1, 0))
        lin = np.asarray(fg)[idx, j].astype(np.int64)
        c = np.stack([lin // (S[1] * S[2]), lin // S[2] % S[1], lin % S[2]], axis=1)
        at = np.minimum(np.maximum(c - T[None, :] // 2, 0), (S - T)[None, :])
        origin = np.where(used[:, None], at, origin)
    return origin.astype(np.int32), used


def crop_torch(x, y, origin, patch):
    """The patches of batch tensors x [n, (Ds,) Hs, Ws, C] and y [n, (Ds,) Hs, Ws, K] (any device)
    at `origin` [n][3] = (d, h, w), `patch` = (D, H, W) (or (H, W)) voxels each: a per-sample
    slice, new tensors.  The whole training transform is
    ``apply_torch(*crop_torch(x, y, origin, patch), code, affine)``."""
    import torch
    org = np.asarray(origin.cpu() if isinstance(origin, torch.Tensor) else origin).reshape(-1, 3)
    n = x.shape[0]
    if len(org) != n or y.shape[0] != n:
        raise ValueError("crop_torch: %d origins for %d images and %d targets" % (len(org), n, y.shape[0]))
    D, H, W = _dims3(patch)
    three_d = x.dim() == 5
    S = tuple(x.shape[1:4]) if three_d else (1,) + tuple(x.shape[1:3])
    if not three_d and D != 1:
        raise ValueError("crop_torch: 2D samples take a patch of depth 1")
    for a, (o, t, s) in enumerate(zip(org.T, (D, H, W), S)):
        if (o < 0).any() or (o + t > s).any():
            raise ValueError("crop_torch: origins of axis %d outside [0, %d]" % (a, s - t))
    out = []
    for src in (x, y):
        parts = []
        for i, (d, h, w) in enumerate(org):
            parts.append(src[i, d:d + D, h:h + H, w:w + W] if three_d else src[i, h:h + H, w:w + W])
        out.append(torch.stack(parts) if parts else src.new_zeros((0,) + ((D, H, W) if three_d else (H, W))
                                                                  + (src.shape[-1],)))
    return out[0], out[1]


# first hash lane of draw_spatial's words: past draw's and draw_crop's, so codes, affines and
# origins are the same with and without rotate / scale
_SPATIAL_LANE = 1 << 17
MAT_ONE = 1 << 16                    # 1.0 in the Q16 of a warp matrix
MAT_MAX = 1 << 18                    # every entry is clamped into [-MAT_MAX, MAT_MAX] before use


def draw_spatial(seed: int, step: int, sample_idx, names, rotate_deg: float = 30.0,
                 scale_a: float = 0.25) -> np.ndarray:
    """mat int32 [n][4] = (a00, a01, a10, a11) in Q16 of the dataset samples `sample_idx` at
    global step `step`: the 2 x 2 matrix that maps an output offset from the patch centre to a
    source offset from it, in the (H, W) plane.  The same counter hash as :func:`draw` with two
    words of its own.  `names`: the --augment string or its parsed names; with `rotate`
    theta = (2 u0 - 1) rotate_deg pi / 180, else 0; with `scale` the zoom z =
    (1 + scale_a) ** (2 u1 - 1), log-uniform in [1 / (1 + a), 1 + a], else 1;
    a00 = a11 = rint(65536 cos(theta) / z), a10 = rint(65536 sin(theta) / z), a01 = -a10."""
    names = parse_augment(names) if isinstance(names, str) else tuple(names)
    idx = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    u = _unit(_hash(seed, step, idx, 2, first=_SPATIAL_LANE))
    theta = (2.0 * u[:, 0] - 1.0) * (float(rotate_deg) * np.pi / 180.0) if "rotate" in names else np.zeros(len(idx))
    z = (1.0 + float(scale_a)) ** (2.0 * u[:, 1] - 1.0) if "scale" in names else np.ones(len(idx))
    c, s = np.rint(MAT_ONE * np.cos(theta) / z), np.rint(MAT_ONE * np.sin(theta) / z)
    return np.stack([c, -s, s, c], axis=1).astype(np.int32)


def mat_of_code(code: int) -> np.ndarray:
    """int32 [4]: the exact warp matrix of in-plane code `code` (0..7): entries 0 or +-65536, so
    warping with it and code 0 is apply_torch with `code`."""
    code = int(code)
    if not 0 <= code < 8:
        raise ValueError("mat_of_code: an in-plane code 0..7, got %r" % (code,))
    sh, sw = (-MAT_ONE if code & FH else MAT_ONE), (-MAT_ONE if code & FW else MAT_ONE)
    return np.array([0, sh, sw, 0] if code & T else [sh, 0, 0, sw], dtype=np.int32)


# first hash lane of draw_spatial3's two out-of-plane words: past the elastic field's lanes (at most
# 2 (2^13 + 3)^2 < 2^28 of them from 2^18 on), so codes, affines, origins, the in-plane angle, the
# zoom and the field are the same with and without rotate3d / scale3d
_SPATIAL3_LANE = 1 << 30


def draw_spatial3(seed: int, step: int, sample_idx, names, rotate_deg: float = 30.0, rotate3d_deg: float = 15.0,
                  scale_a: float = 0.25) -> np.ndarray:
    """mat int32 [n][9]: the row-major 3 x 3 matrix in Q16 over the axes (d, h, w) that maps an
    output offset from the patch centre to a source offset from it.  theta0, the in-plane angle
    about the depth axis, and the zoom z come from draw_spatial's two words and are formed as it
    forms them: theta0 with `rotate` or `rotate3d`, else 0; z with `scale` or `scale3d`, else 1.
    theta1 (in the (d, w) plane, about the h axis) and theta2 (in the (d, h) plane, about the w
    axis) are (2 u - 1) rotate3d_deg pi / 180 of two words of their own with `rotate3d`, else 0.
    With Rd(t) = [[1,0,0],[0,c,-s],[0,s,c]], Rh(t) = [[c,0,-s],[0,1,0],[s,0,c]] and
    Rw(t) = [[c,-s,0],[s,c,0],[0,0,1]]: R = Rd(theta0) Rh(theta1) Rw(theta2) in float64 and
    mat[i][j] = rint(65536 R[i][j] / z_j), z_h = z_w = z, z_d = z with `scale3d` and 1 with `scale`.
    With theta1 = theta2 = 0 and z_d = 1 the lower-right 2 x 2 block is draw_spatial's integers,
    row 0 is (65536, 0, 0) and column 0 below it is 0."""
    names = parse_augment(names) if isinstance(names, str) else tuple(names)
    idx = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    n = len(idx)
    u = _unit(_hash(seed, step, idx, 2, first=_SPATIAL_LANE))
    rot = "rotate" in names or "rotate3d" in names
    theta0 = (2.0 * u[:, 0] - 1.0) * (float(rotate_deg) * np.pi / 180.0) if rot else np.zeros(n)
    z = (1.0 + float(scale_a)) ** (2.0 * u[:, 1] - 1.0) if "scale" in names or "scale3d" in names else np.ones(n)
    if "rotate3d" in names:
        u3 = _unit(_hash(seed, step, idx, 2, first=_SPATIAL3_LANE))
        theta1 = (2.0 * u3[:, 0] - 1.0) * (float(rotate3d_deg) * np.pi / 180.0)
        theta2 = (2.0 * u3[:, 1] - 1.0) * (float(rotate3d_deg) * np.pi / 180.0)
    else:
        theta1 = theta2 = np.zeros(n)
    return mat3_of(theta0, theta1, theta2, z, z if "scale3d" in names else np.ones(n))


def mat3_of(theta0, theta1, theta2, z, zd) -> np.ndarray:
    """int32 [n][9]: draw_spatial3's matrix of the angles (radians) and the zooms z (h and w) and zd
    (d), arrays [n] or scalars."""
    t0, t1, t2, z, zd = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype=np.float64))
                                              for v in (theta0, theta1, theta2, z, zd)))
    n = len(t0)
    one, zero = np.ones(n), np.zeros(n)

    def m(rows):
        return np.stack([np.stack(r, axis=1) for r in rows], axis=1)

    c, s = np.cos(t0), np.sin(t0)
    rd = m([[one, zero, zero], [zero, c, -s], [zero, s, c]])
    c, s = np.cos(t1), np.sin(t1)
    rh = m([[c, zero, -s], [zero, one, zero], [s, zero, c]])
    c, s = np.cos(t2), np.sin(t2)
    rw = m([[c, -s, zero], [s, c, zero], [zero, zero, one]])
    r = np.einsum("nij,njk,nkl->nil", rd, rh, rw)
    zj = np.stack([zd, z, z], axis=1)[:, None, :]
    return (np.rint(MAT_ONE * r / zj) + 0.0).astype(np.int32).reshape(n, 9)


def embed_mat3(mat) -> np.ndarray:
    """int [n][9]: the 3 x 3 matrix that leaves depth alone and acts on (h, w) as `mat` int [n][4]."""
    m = np.asarray(mat).reshape(-1, 4)
    out = np.zeros((len(m), 9), dtype=m.dtype)
    out[:, 0] = MAT_ONE
    out[:, [4, 5, 7, 8]] = m
    return out


def warp3_torch(x, y, origin, patch, mat3, disp=None):
    """warp_torch with depth rotated, zoomed and interpolated: the resampled patches of 5-D batch
    tensors x [n, Ds, Hs, Ws, C] and y [n, Ds, Hs, Ws, K] (any device), `patch` = (D, H, W) voxels
    at `origin` [n][3] (None: 0; clamped into the sample), read through `mat3` int [n][9]
    (draw_spatial3; entries clamped into [-2^18, 2^18]).  `disp`: None, or (field, S) -- an elastic
    field int [n][Nh][Nw][2] (draw_elastic) with cells of S patch pixels, whose displacement
    (elastic_disp, a lattice over (h', w'), the same in every patch slice) is added to Qh and Qw.

    With t = 2 d - (D-1), u = 2 h - (H-1), v = 2 w - (W-1) at patch voxel (d, h, w):
    Qd = (od << 17) + (D-1) 65536 + m00 t + m01 u + m02 v, Qh and Qw alike from rows 1 and 2, 64-bit,
    in 2^-17 voxel.  Image: id = Qd >> 17, fd = Qd & 0x1FFFF; s0 and s1 are warp_torch's bilinear
    value in the slices id and id + 1 (a tap whose slice, row or column is outside the stored
    volume is 0) and the result is s0 wd0 + s1 wd1, wd1 = fd 2^-17, wd0 = (131072 - fd) 2^-17: two
    products and one sum, each rounded to fp32 once.  Target: y at the nearest voxel
    ((Qd + 65536) >> 17, (Qh + 65536) >> 17, (Qw + 65536) >> 17), 0 outside.  The whole training
    transform is ``apply_torch(*warp3_torch(...), code, affine)`` and the oracle of
    ``gather_batch_warp3`` (``csrc/kernels/gather_resample.h``)."""
    import torch
    if x.dim() != 5:
        raise ValueError("warp3_torch: 5-D samples [n, Ds, Hs, Ws, C], got %d-D" % x.dim())
    m = np.asarray(mat3.cpu() if isinstance(mat3, torch.Tensor) else mat3)
    if m.ndim != 2 or m.shape[1] != 9:
        raise ValueError("warp3_torch: matrices int [n][9], got %r" % (tuple(m.shape),))
    fn = None
    if disp is not None:
        field, S = disp
        fl = field.cpu() if isinstance(field, torch.Tensor) else field
        if len(fl) != x.shape[0]:
            raise ValueError("warp3_torch: %d fields for %d images" % (len(fl), x.shape[0]))
        fn = lambda n, H, W, dev: tuple(d.view(n, H, W) for d in elastic_disp(fl, (H, W), S, dev))
    return _resample("warp3_torch", x, y, origin, patch, m, fn)


def warp_torch(x, y, origin, patch, mat):
    """The resampled patches of batch tensors x [n, (Ds,) Hs, Ws, C] and y [n, (Ds,) Hs, Ws, K]
    (any device): `patch` = (D, H, W) (or (H, W)) voxels at `origin` [n][3] = (d, h, w) (None: 0;
    clamped into the sample), read through `mat` int [n][4] (draw_spatial; entries clamped into
    [-2^18, 2^18]).  New tensors [n, (D,) H, W, C / K]: the image bilinear, the target nearest,
    both zero outside the stored image; depth is neither rotated nor interpolated.

    The geometry is integer: with u = 2 h - (H-1), v = 2 w - (W-1),
    Qh = (oh << 17) + (H-1) 65536 + a00 u + a01 v and Qw = (ow << 17) + (W-1) 65536 + a10 u + a11 v
    are source coordinates in 2^-17 pixel.  Image: ih = Qh >> 17, fh = Qh & 0x1FFFF, taps
    p_ij = x[ih + i][iw + j] (0 outside), weights wh1 = fh 2^-17, wh0 = (131072 - fh) 2^-17,
    r0 = p00 ww0 + p01 ww1, r1 = p10 ww0 + p11 ww1, value = r0 wh0 + r1 wh1 -- one fp32 tensor
    op per product and per sum, each rounding once.  Target: y at ((Qh + 65536) >> 17,
    (Qw + 65536) >> 17).  The whole training transform is
    ``apply_torch(*warp_torch(x, y, origin, patch, mat), code, affine)`` straight from the stored
    samples -- taps outside the patch rectangle read the stored image -- and the oracle of
    ``csrc/kernels/gather_resample.h``."""
    return _resample("warp_torch", x, y, origin, patch, mat, None)


def _resample(who, x, y, origin, patch, mat, disp):
    """warp_torch's and warp3_torch's body; `mat` None is the identity, int [n][4] the in-plane
    matrix (depth is then a plain slice) and int [n][9] the matrix over (d, h, w); `disp` = None or a
    function (n, H, W, device) -> (dh, dw) int64 [n, H, W] added to the source coordinates Qh, Qw
    (elastic_torch)."""
    import torch
    n = x.shape[0]
    D, H, W = _dims3(patch)
    three_d = x.dim() == 5
    Ds, Hs, Ws = tuple(x.shape[1:4]) if three_d else (1,) + tuple(x.shape[1:3])
    if not three_d and D != 1:
        raise ValueError("%s: 2D samples take a patch of depth 1" % who)
    if D > Ds or H > Hs or W > Ws:
        raise ValueError("%s: patch %r exceeds the stored sample %r" % (who, (D, H, W), (Ds, Hs, Ws)))
    if mat is None:
        mat = np.tile(np.array([MAT_ONE, 0, 0, MAT_ONE], dtype=np.int64), (n, 1))
    m = np.asarray(mat.cpu() if isinstance(mat, torch.Tensor) else mat)
    full = m.ndim == 2 and m.shape[1] == 9           # the 3 x 3 matrix: depth is resampled too
    m = m.reshape(-1, 9 if full else 4).astype(np.int64)
    if origin is None:
        org = np.zeros((n, 3), dtype=np.int64)
    else:
        org = np.asarray(origin.cpu() if isinstance(origin, torch.Tensor) else origin).reshape(-1, 3).astype(np.int64)
    if len(m) != n or len(org) != n or y.shape[0] != n:
        raise ValueError("%s: %d matrices and %d origins for %d images and %d targets"
                         % (who, len(m), len(org), n, y.shape[0]))
    dev = x.device
    m = torch.from_numpy(np.clip(m, -MAT_MAX, MAT_MAX)).to(dev)
    org = torch.from_numpy(np.clip(org, 0, np.array([Ds - D, Hs - H, Ws - W], dtype=np.int64)[None, :])).to(dev)
    u = (2 * torch.arange(H, dtype=torch.int64, device=dev) - (H - 1)).view(1, 1, H, 1)
    v = (2 * torch.arange(W, dtype=torch.int64, device=dev) - (W - 1)).view(1, 1, 1, W)
    dd = torch.arange(D, dtype=torch.int64, device=dev).view(1, D, 1, 1)
    a = [m[:, e].view(n, 1, 1, 1) for e in range(m.shape[1])]
    oc = [org[:, e].view(n, 1, 1, 1) << 17 for e in range(3)]
    if full:
        t = 2 * dd - (D - 1)
        qd = oc[0] + (D - 1) * 65536 + a[0] * t + a[1] * u + a[2] * v
        qh = oc[1] + (H - 1) * 65536 + a[3] * t + a[4] * u + a[5] * v
        qw = oc[2] + (W - 1) * 65536 + a[6] * t + a[7] * u + a[8] * v
    else:
        qh = oc[1] + (H - 1) * 65536 + a[0] * u + a[1] * v
        qw = oc[2] + (W - 1) * 65536 + a[2] * u + a[3] * v
    if disp is not None:
        dh, dw = disp(n, H, W, dev)
        qh, qw = qh + dh.view(n, 1, H, W), qw + dw.view(n, 1, H, W)
    shape = (n, D, H, W)

    def taps(src, sl, r, c):
        """src [n, (Ds,) Hs, Ws, C] at slices sl, rows r and columns c (each broadcasts to
        [n, D, H, W]): [n, D, H, W, C], 0 outside the stored volume."""
        C = src.shape[-1]
        ok = ((sl >= 0) & (sl < Ds) & (r >= 0) & (r < Hs) & (c >= 0) & (c < Ws)).expand(shape)
        lin = ((sl.clamp(0, Ds - 1) * Hs + r.clamp(0, Hs - 1)) * Ws + c.clamp(0, Ws - 1)).expand(shape)
        g = src.reshape(n, Ds * Hs * Ws, C).gather(1, lin.reshape(n, D * H * W, 1).expand(n, D * H * W, C))
        return torch.where(ok.unsqueeze(-1), g.view(shape + (C,)), torch.zeros((), dtype=src.dtype, device=dev))

    ih, iw = qh >> 17, qw >> 17
    fh, fw = qh & 0x1FFFF, qw & 0x1FFFF
    wh1, wh0 = (fh.float() * 2.0 ** -17).unsqueeze(-1), ((131072 - fh).float() * 2.0 ** -17).unsqueeze(-1)
    ww1, ww0 = (fw.float() * 2.0 ** -17).unsqueeze(-1), ((131072 - fw).float() * 2.0 ** -17).unsqueeze(-1)

    def bilinear(sl):
        r0 = taps(x, sl, ih, iw) * ww0 + taps(x, sl, ih, iw + 1) * ww1
        r1 = taps(x, sl, ih + 1, iw) * ww0 + taps(x, sl, ih + 1, iw + 1) * ww1
        return r0 * wh0 + r1 * wh1

    if full:
        idp, fd = qd >> 17, qd & 0x1FFFF
        wd1, wd0 = (fd.float() * 2.0 ** -17).unsqueeze(-1), ((131072 - fd).float() * 2.0 ** -17).unsqueeze(-1)
        xo = bilinear(idp) * wd0 + bilinear(idp + 1) * wd1
        yo = taps(y, (qd + 65536) >> 17, (qh + 65536) >> 17, (qw + 65536) >> 17)
    else:
        sl = org[:, 0].view(n, 1, 1, 1) + dd             # the D slices of every sample: always inside
        xo = bilinear(sl)
        yo = taps(y, sl, (qh + 65536) >> 17, (qw + 65536) >> 17)
    if not three_d:
        xo, yo = xo.squeeze(1), yo.squeeze(1)
    return xo.contiguous(), yo.contiguous()


# first hash lane of draw_elastic's words: past draw's, draw_crop's and draw_spatial's, so codes,
# affines, origins and matrices are the same with and without elastic
_ELASTIC_LANE = 1 << 18
FIELD_MAX = 1 << 22                  # every field entry is clamped into [-FIELD_MAX, FIELD_MAX] (32 pixels) before use
# standard deviation of the sum of a word's four 16-bit fields: each is uniform on 0..65535
_ELASTIC_SD = float(np.sqrt(((1 << 32) - 1) / 3.0))


def elastic_log2(S) -> int:
    """s = log2 S of a control-lattice cell side S in {8, 16, 32, 64}; ValueError otherwise."""
    S = int(S)
    if S not in (8, 16, 32, 64):
        raise ValueError("elastic cell side: 8, 16, 32 or 64 patch pixels, got %r" % (S,))
    return S.bit_length() - 1


def elastic_nodes(side: int, S: int) -> int:
    """Control nodes along a patch axis of `side` pixels: ((side - 1) >> s) + 3."""
    return ((int(side) - 1) >> elastic_log2(S)) + 3


def _hw(patch_hw) -> Tuple[int, int]:
    if isinstance(patch_hw, (int, np.integer)):
        return int(patch_hw), int(patch_hw)
    return tuple(int(v) for v in tuple(patch_hw)[-2:])


def draw_elastic(seed: int, step: int, sample_idx, patch_hw, a: float = 4.0, S: int = 32) -> np.ndarray:
    """field int32 [n][Nh][Nw][2] of the dataset samples `sample_idx` at global step `step`: the
    displacement of control node (i, j) of the patch's quadratic B-spline lattice along h (entry 0)
    and w (entry 1), in 2^-17 pixel of the stored image.  `patch_hw` = (H, W) (or one side) of the
    patch, N = ((side - 1) >> log2 S) + 3 nodes per axis, cells of S patch pixels.  The same
    counter hash as :func:`draw` with words of its own, one per entry in (i, j, c) order.  A word
    becomes a near-Gaussian without libm: t = the sum of its four 16-bit fields, g = (t - 131070)
    / sqrt((2^32 - 1) / 3), entry = clip(rint(131072 a g), -2a 131072, 2a 131072): standard
    deviation `a` pixels, truncated at two of them."""
    H, W = _hw(patch_hw)
    nh, nw = elastic_nodes(H, S), elastic_nodes(W, S)
    idx = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    h = _hash(seed, step, idx, nh * nw * 2, first=_ELASTIC_LANE)
    m = np.uint64(0xFFFF)
    t = ((h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))).astype(np.int64)
    g = (t - 131070).astype(np.float64) / _ELASTIC_SD
    lim = 2.0 * float(a) * 131072.0
    return np.clip(np.rint(131072.0 * float(a) * g), -lim, lim).astype(np.int32).reshape(len(idx), nh, nw, 2)


def elastic_disp(field, patch_hw, S: int, device=None):
    """(dh, dw) int64 tensors [n, H, W]: the displacement of every patch pixel (h', w') under
    `field` int [n][Nh][Nw][2] (entries clamped into [-2^22, 2^22]), in 2^-17 pixel.  With
    ci = h' >> s, t = h' & (S - 1) the integer quadratic B-spline weights are
    wh = [(S - t)^2, -2 t^2 + 2 S t + S^2, t^2] (sum 2 S^2), ww alike from w', and
    d_c = (sum_a wh[a] sum_b ww[b] f[ci + a][cj + b][c]) >> (2 + 4 s) -- an arithmetic shift of an
    int64 sum below 2^48 -- so a constant field displaces by exactly that constant."""
    import torch
    s = elastic_log2(S)
    H, W = _hw(patch_hw)
    f = torch.as_tensor(np.asarray(field.cpu() if isinstance(field, torch.Tensor) else field).astype(np.int64))
    if f.dim() != 4 or tuple(f.shape[1:]) != (elastic_nodes(H, S), elastic_nodes(W, S), 2):
        raise ValueError("elastic field: [n][%d][%d][2] for a %d x %d patch at cell %d, got %r"
                         % (elastic_nodes(H, S), elastic_nodes(W, S), H, W, S, tuple(f.shape)))
    f = f.clamp(-FIELD_MAX, FIELD_MAX).to(device if device is not None else "cpu")
    n, dev = f.shape[0], f.device

    def weights(side):
        p = torch.arange(side, dtype=torch.int64, device=dev)
        t = p & (S - 1)
        return p >> s, torch.stack([(S - t) * (S - t), -2 * t * t + 2 * S * t + S * S, t * t])

    ci, wh = weights(H)
    cj, ww = weights(W)
    acc = torch.zeros(n, H, W, 2, dtype=torch.int64, device=dev)
    for a in range(3):
        rows = f[:, ci + a]                                       # [n, H, Nw, 2]
        inner = torch.zeros(n, H, W, 2, dtype=torch.int64, device=dev)
        for b in range(3):
            inner = inner + ww[b].view(1, 1, W, 1) * rows[:, :, cj + b]
        acc = acc + wh[a].view(1, H, 1, 1) * inner
    d = acc >> (2 + 4 * s)
    return d[..., 0].contiguous(), d[..., 1].contiguous()


def elastic_torch(x, y, origin, patch, mat, field, S: int):
    """warp_torch with a smooth per-pixel displacement: the patches of batch tensors x [n, (Ds,) Hs,
    Ws, C] and y (any device) at `origin` (None: 0), read through `mat` int [n][4] (None: the
    identity) at source coordinates Qh = (warp_torch's Qh) + d_0, Qw = (warp_torch's Qw) + d_1 with
    (d_0, d_1) = :func:`elastic_disp` of `field` int [n][Nh][Nw][2] (draw_elastic) at the patch
    pixel.  From Q on everything is warp_torch's: taps, weights, one fp32 rounding per op, nearest
    target, zero outside the stored image; every depth slice of a sample uses the same field.
    The whole training transform is ``apply_torch(*elastic_torch(...), code, affine)`` -- the
    displacement is indexed by the patch pixel before the flip / transpose code -- and the oracle
    of ``csrc/kernels/gather_resample.h``."""
    import torch
    fl = field.cpu() if isinstance(field, torch.Tensor) else field
    if len(fl) != x.shape[0]:
        raise ValueError("elastic_torch: %d fields for %d images" % (len(fl), x.shape[0]))
    return _resample("elastic_torch", x, y, origin, patch, mat,
                     lambda n, H, W, dev: tuple(d.view(n, H, W) for d in elastic_disp(fl, (H, W), S, dev)))


def inverse_code(code: int) -> int:
    """The code that undoes `code` (the two quarter turns swap; every other code is an involution)."""
    if code & T and bool(code & FH) != bool(code & FW):
        return code ^ (FH | FW)
    return code


def apply_torch(x, y, code, affine=None):
    """The transform on batch tensors x [n, (D,) H, W, C] and y [n, (D,) H, W, K] (any device):
    new tensors, the inputs are left alone.  The affine is evaluated in float64 and rounded
    to fp32 once."""
    import torch
    code = np.asarray(code.cpu() if isinstance(code, torch.Tensor) else code).reshape(-1)
    n = x.shape[0]
    if len(code) != n or y.shape[0] != n:
        raise ValueError("apply_torch: %d codes for %d images and %d targets" % (len(code), n, y.shape[0]))
    hd, wd = x.dim() - 3, x.dim() - 2
    if x.shape[hd] != x.shape[wd] and (code & T).any():
        raise ValueError("apply_torch: the H / W swap needs square images")
    if x.dim() == 4 and (code & FD).any():
        raise ValueError("apply_torch: the D flip needs 3D samples")
    xo, yo = torch.empty_like(x), torch.empty_like(y)
    for c in np.unique(code):
        sel = torch.from_numpy(np.nonzero(code == c)[0]).to(x.device)
        flips = [d for bit, d in ((FH, hd), (FW, wd), (FD, 1)) if c & bit]
        for src, dst in ((x, xo), (y, yo)):
            t = src.index_select(0, sel)
            if flips:
                t = t.flip(flips)               # the flips act on the source ...
            if c & T:
                t = t.transpose(hd, wd)         # ... and the swap on what they leave
            dst.index_copy_(0, sel, t.contiguous())
    if affine is not None:
        af = torch.as_tensor(affine).to(x.device).double()
        af = af.view((n,) + (1,) * (x.dim() - 2) + (af.shape[1], 2))
        xo = (xo.double() * af[..., 0] + af[..., 1]).to(x.dtype)
    return xo, yo


def tta_codes(spec, dims: int) -> Tuple[int, ...]:
    """The transform codes of test-time augmentation `spec` (the --eval_tta string or its
    parsed names): `flip` every subset of the flips of the sample's axes, `rot90` the four
    quarter turns, both every code; ascending with the identity LAST (the executors' identity
    pass leaves the stored target behind).  M = len is a power of two (1 / M is exact); () is off."""
    names = parse_tta(spec) if isinstance(spec, str) else tuple(spec)
    flip, rot = "flip" in names, "rot90" in names
    if flip and rot:
        codes = range(16 if dims == 3 else 8)
    elif flip:
        bits = FW | FH | (FD if dims == 3 else 0)
        codes = [c for c in range(16) if not c & ~bits]
    elif rot:
        codes = ROT90_CODES
    else:
        return ()
    return tuple(sorted(c for c in codes if c)) + (0,)


def tta_mean_torch(predict_fn, x, codes):
    """Mean over `codes` (tta_codes: the identity last) of predict_fn's probabilities of the
    transformed batch x [n, (D,) H, W, C], each brought back by its inverse transform.  The
    arithmetic is the HIP path's (kernels/tta.h), in its order: acc = unaug(p_c0);
    acc = acc + unaug(p_ci) for each later code; p = (acc + p_identity) * (1 / M) in fp32."""
    codes = tuple(int(c) for c in codes)
    if len(codes) < 2 or codes[-1] != 0 or 0 in codes[:-1] or len(codes) & (len(codes) - 1):
        raise ValueError("tta_mean_torch: a power of two >= 2 of codes with the identity last, got %r" % (codes,))
    n = x.shape[0]
    acc = None
    for c in codes[:-1]:
        p = predict_fn(apply_torch(x, x, [c] * n)[0]).float()
        u = apply_torch(p, p, [inverse_code(c)] * n)[0]
        acc = u if acc is None else acc + u
    return (acc + predict_fn(x).float()) * (1.0 / len(codes))


def make_aug(cfg, step: int) -> Optional[Callable[[Sequence[int]], Tuple[np.ndarray, Optional[np.ndarray]]]]:
    """The per-step callable a DeviceFeeder takes (dataset sample indices -> parameters),
    or None when --augment is off.  With `rotate` or `scale` named the parameters gain the warp
    matrices as a last item: (code, affine, mat).  With `elastic` named they are (code, affine,
    mat or None, field): the matrices' slot is always there, the field (draw_elastic) comes last.
    With `rotate3d` or `scale3d` named the matrices are draw_spatial3's [n][9] ones."""
    names = parse_augment(cfg.augment)
    if not names:
        return None
    side = (cfg.img_size, cfg.img_size)

    def fn(idx):
        out = draw(cfg.seed, step, idx, names, cfg.in_channels, cfg.dims, cfg.augment_intensity)
        spatial = has_spatial(names)
        if spatial:
            out = out + (_draw_mat(cfg, step, idx, names),)
        if "elastic" in names:
            out = out + (() if spatial else (None,)) + (
                draw_elastic(cfg.seed, step, idx, side, cfg.augment_elastic, cfg.augment_elastic_cell),)
        return out

    return fn


def has_spatial(names) -> bool:
    """Whether the --augment names hold a transform that resamples the image through a matrix
    (rotate, scale, rotate3d, scale3d)."""
    return any(t in SPATIAL_NAMES or t in SPATIAL3_NAMES for t in names)


def has_spatial3(names) -> bool:
    """Whether the --augment names hold a transform whose matrix is the 3 x 3 one (rotate3d, scale3d)."""
    return any(t in SPATIAL3_NAMES for t in names)


def _draw_mat(cfg, step: int, idx, names) -> np.ndarray:
    """The matrix slot of make_aug / make_crop_aug: [n][9] with a 3D name, else draw_spatial's [n][4]."""
    if has_spatial3(names):
        return draw_spatial3(cfg.seed, step, idx, names, cfg.augment_rotate, cfg.augment_rotate3d, cfg.augment_scale)
    return draw_spatial(cfg.seed, step, idx, names, cfg.augment_rotate, cfg.augment_scale)


def make_crop_aug(cfg, step: int, stored, table=None):
    """make_aug's sibling for --crop: dataset sample indices -> (code, affine, origin).  The
    codes are all zero and the affine None when --augment is off; the origins are draw_crop's.
    With `rotate` or `scale` named: (code, affine, origin, mat).  With `elastic` named:
    (code, affine, origin, mat or None, field).  With `rotate3d` or `scale3d` named the matrices
    are draw_spatial3's [n][9] ones."""
    mode, p_fg = parse_crop(cfg.crop)
    names = parse_augment(cfg.augment)
    patch = (cfg.img_size,) * 3 if cfg.dims == 3 else (1, cfg.img_size, cfg.img_size)

    def fn(idx):
        code, affine = draw(cfg.seed, step, idx, names, cfg.in_channels, cfg.dims, cfg.augment_intensity)
        origin, _ = draw_crop(cfg.seed, step, idx, stored, patch, mode, p_fg, table)
        mat = _draw_mat(cfg, step, idx, names) if has_spatial(names) else None
        if "elastic" in names:
            return code, affine, origin, mat, draw_elastic(cfg.seed, step, idx, patch[1:], cfg.augment_elastic,
                                                           cfg.augment_elastic_cell)
        if mat is not None:
            return code, affine, origin, mat
        return code, affine, origin

    return fn

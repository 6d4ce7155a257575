"""Sliding-window inference: geometry and the torch oracle.

An image larger (or smaller) than the model's input is cut into overlapping tiles of the
model's size, every tile is predicted, the tile predictions are blended with a weight map
and the sum is divided by the summed weights.  This module is the definition: the HIP
kernels (`csrc/kernels/sliding.h`) and both backends are tested against it, bit for bit.

Tile        T = (Td, Th, Tw): (1, S, S) in 2D, (S, S, S) in 3D, S the model's `img_size`.
            The image is (D, H, W), D = 1 in 2D; any axis may be smaller than the tile.
Stride      s = T - floor(overlap * T) per axis, overlap in [0, 0.75]; 1 on an axis with T = 1.
Origins     of an axis of length L: [0] if L <= T, else n = ceil((L - T) / s) + 1 origins
            o_i = min(i * s, L - T): the last tile is clamped to end at the edge.
Tile order  image outermost, then the grid indices (id, ih, iw), iw fastest.  Tile t of a
            chunk of images sits in slot t % B of batch t // B; the slots of the last batch
            past the last tile hold zeros.
Weights     fp32 [Td][Th][Tw]: `constant` all ones; `gaussian` the outer product of
            g[i] = exp(-0.5 ((i - (T - 1) / 2) / (0.125 T))^2) per axis, formed in float64 and
            rounded once (smallest value at 128^3: 5.5e-11, a normal fp32 number: no clamp).
Blend       acc = 0; for tiles in ascending order acc[region] = acc[region] + (w * p_tile):
            an fp32 multiplication, then an fp32 addition (never an fma), the part of a tile
            past an image smaller than the tile dropped.  wsum is the same sum with p = 1,
            the result acc / wsum, a true fp32 division.

fp32 rounding is monotone and both sums run in the same order, so 0 <= acc <= wsum whenever
0 <= p <= 1: the result lies in [0, 1], p == 1 gives exactly 1, and a constant blend of an
image of exactly the tile size returns the tile prediction bit for bit.
"""

import math
from typing import Callable, List, Sequence, Tuple

import torch

BLENDS = ("constant", "gaussian")
MAX_OVERLAP = 0.75


def check_overlap(overlap) -> float:
    o = float(overlap)
    if not 0.0 <= o <= MAX_OVERLAP:          # (NaN fails both comparisons)
        raise ValueError("sliding window: overlap must lie in [0, %g], got %r" % (MAX_OVERLAP, overlap))
    return o


def check_blend(blend) -> str:
    if blend not in BLENDS:
        raise ValueError("sliding window: blend must be one of %s, got %r" % (" | ".join(BLENDS), blend))
    return blend


def tile_shape(img_size: int, dims: int) -> Tuple[int, int, int]:
    s = int(img_size)
    return (s, s, s) if dims == 3 else (1, s, s)


def strides(T: Sequence[int], overlap: float) -> Tuple[int, ...]:
    o = check_overlap(overlap)
    return tuple(1 if t == 1 else t - int(math.floor(o * t)) for t in T)


def tile_origins(L: int, T: int, s: int) -> List[int]:
    if L < 1 or T < 1 or s < 1:
        raise ValueError("tile_origins: L, T, s >= 1, got %r" % ((L, T, s),))
    if L <= T:
        return [0]
    return [min(i * s, L - T) for i in range(-(-(L - T) // s) + 1)]


def grid_origins(dims: Sequence[int], T: Sequence[int], stride: Sequence[int]) -> List[List[int]]:
    return [tile_origins(int(L), int(t), int(s)) for L, t, s in zip(dims, T, stride)]


def tiles_per_image(dims, T, stride) -> int:
    od, oh, ow = grid_origins(dims, T, stride)
    return len(od) * len(oh) * len(ow)


def tile_list(dims, T, stride) -> List[Tuple[int, int, int]]:
    """The origins (od, oh, ow) of one image's tiles in tile order."""
    od, oh, ow = grid_origins(dims, T, stride)
    return [(a, b, c) for a in od for b in oh for c in ow]


def weight_map(T: Sequence[int], blend: str) -> torch.Tensor:
    check_blend(blend)
    if blend == "constant":
        return torch.ones(tuple(int(t) for t in T), dtype=torch.float32)
    g = []
    for t in T:
        i = torch.arange(int(t), dtype=torch.float64)
        g.append(torch.exp(-0.5 * ((i - (t - 1) / 2.0) / (0.125 * t)) ** 2))
    w = g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    return w.to(torch.float32)


def _clip(o, L, T):
    """(image slice, tile slice) of one axis of a tile at origin o."""
    n = min(T, L - o)
    return slice(o, o + n), slice(0, n)


def weight_sum(dims, T, stride, blend: str) -> torch.Tensor:
    """fp32 [D][H][W]: the blend of p == 1, in the blend's own order."""
    w = weight_map(T, blend)
    acc = torch.zeros(tuple(int(v) for v in dims), dtype=torch.float32)
    for o in tile_list(dims, T, stride):
        (i0, t0), (i1, t1), (i2, t2) = (_clip(o[a], dims[a], T[a]) for a in range(3))
        acc[i0, i1, i2] = acc[i0, i1, i2] + w[t0, t1, t2]
    return acc


def _as5(x: torch.Tensor) -> torch.Tensor:
    if x.dim() == 4:
        return x.unsqueeze(1)
    if x.dim() != 5:
        raise ValueError("sliding window: images are [n, (D,) H, W, C], got shape %r" % (tuple(x.shape),))
    return x


def extract_tiles_torch(x: torch.Tensor, T, stride, B: int, t0: int, nt: int) -> torch.Tensor:
    """One staging batch [B][Td][Th][Tw][C] of the images x [N, (D,) H, W, C]: slot b < nt
    holds tile t0 + b, the other slots and the positions past the image are zeros."""
    x = _as5(x)
    dims = tuple(x.shape[1:4])
    tl = tile_list(dims, T, stride)
    out = x.new_zeros((B,) + tuple(int(t) for t in T) + (x.shape[-1],))
    if not (0 <= t0 and 0 <= nt <= B and t0 + nt <= x.shape[0] * len(tl)):
        raise ValueError("extract_tiles_torch: tiles [%d, %d) outside the grid" % (t0, t0 + nt))
    for b in range(nt):
        n, r = divmod(t0 + b, len(tl))
        (i0, s0), (i1, s1), (i2, s2) = (_clip(tl[r][a], dims[a], T[a]) for a in range(3))
        out[b, s0, s1, s2] = x[n, i0, i1, i2]
    return out


def blend_tiles_torch(p_tiles: torch.Tensor, acc: torch.Tensor, T, stride, blend: str, t0: int = 0,
                      w: torch.Tensor = None) -> torch.Tensor:
    """acc [N, (D,) H, W, K] += the weighted tiles p_tiles [nt, (Td,) Th, Tw, K] = tiles
    t0 .. t0 + nt - 1, in ascending order and in place: acc = acc + (w * p)."""
    a5 = _as5(acc)
    p5 = _as5(p_tiles)
    dims = tuple(a5.shape[1:4])
    tl = tile_list(dims, T, stride)
    if w is None:
        w = weight_map(T, blend).to(acc.device)
    for b in range(p5.shape[0]):
        n, r = divmod(t0 + b, len(tl))
        (i0, s0), (i1, s1), (i2, s2) = (_clip(tl[r][a], dims[a], T[a]) for a in range(3))
        prod = w[s0, s1, s2].unsqueeze(-1) * p5[b, s0, s1, s2]
        a5[n, i0, i1, i2] = a5[n, i0, i1, i2] + prod
    return acc


def finish_torch(acc: torch.Tensor, wsum: torch.Tensor) -> torch.Tensor:
    """acc [N, (D,) H, W, K] / wsum [D][H][W]: the blended prediction."""
    a5 = _as5(acc)
    return (a5 / wsum.to(acc.device)[None, ..., None]).view(acc.shape)


def sliding_predict_torch(predict_fn: Callable[[torch.Tensor], torch.Tensor], x: torch.Tensor, T, B: int,
                          overlap: float = 0.5, blend: str = "gaussian") -> torch.Tensor:
    """The whole loop over the images x [N, (D,) H, W, C]: extraction, batches of B tiles in
    slot order with the zero-padded last batch, `predict_fn` per batch ([B, (Td,) Th, Tw, C] ->
    [B, (Td,) Th, Tw, K]), blend and division.  Returns fp32 [N, (D,) H, W, K]."""
    check_blend(blend)
    stride = strides(T, overlap)
    two_d = x.dim() == 4
    x5 = _as5(x)
    N, dims = x5.shape[0], tuple(x5.shape[1:4])
    total = N * tiles_per_image(dims, T, stride)
    w = weight_map(T, blend).to(x.device)
    acc = None
    for t0 in range(0, total, B):
        nt = min(B, total - t0)
        xb = extract_tiles_torch(x5, T, stride, B, t0, nt)
        p = predict_fn(xb[:, 0] if two_d else xb).to(torch.float32)
        if acc is None:
            acc = torch.zeros((N,) + dims + (p.shape[-1],), dtype=torch.float32, device=p.device)
            w = w.to(p.device)
        blend_tiles_torch(_as5(p)[:nt], acc, T, stride, blend, t0, w=w)
    out = finish_torch(acc, weight_sum(dims, T, stride, blend))
    return out[:, 0] if two_d else out

"""Per-class and per-case segmentation metrics from per-(sample, class) statistics.

``stats[n][k] = {I, St, Sp, TP, FP, FN}`` of sample n and class k, with ``t`` the target
and ``p`` the probability:

====  ==============================
slot  value
====  ==============================
0     ``I  = sum t p``
1     ``St = sum t``
2     ``Sp = sum p``
3     ``TP = #(p >= thr and t >= 0.5)``
4     ``FP = #(p >= thr and t <  0.5)``
5     ``FN = #(p <  thr and t >= 0.5)``
====  ==============================

``TN = S - TP - FP - FN`` (S pixels or voxels per sample) is not stored.  The native
executors produce the array with one HIP launch (``csrc/kernels/seg_stats.h``);
:func:`case_stats_torch` is the same array from torch ops -- the ATen backend's
implementation and the oracle of the kernel tests.  The threshold is compared in fp32
(``p`` is fp32 on every path), so ``p == float32(thr)`` counts as positive.

The metric definitions (all float64 on the host):

* ``dice[k]``: the reference's soft Dice with smoothing 1 (`model.py:4-21`) on the sums
  over the given samples, ``(2 sum_n I + 1) / (sum_n St + sum_n Sp + 1)``;
* ``case_dice[k]``: mean over cases of the thresholded ``2 TP / (2 TP + FP + FN)``; a case
  with empty target and empty prediction scores 1.0 (the BraTS convention);
* ``sensitivity[k] = TP / (TP + FN)``, ``specificity[k] = TN / (TN + FP)``, pooled over the
  cases (micro-average); a zero denominator gives ``nan`` (logged as JSON ``null``).
"""

import math
from typing import Dict, Optional

import numpy as np
import torch

NSLOT = 6
SMOOTH = 1.0


@torch.no_grad()
def case_stats_torch(prob: torch.Tensor, target: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """``[N][K][6]`` float64 from ``prob`` / ``target`` of shape ``[N, ..., K]``."""
    n, k = prob.shape[0], prob.shape[-1]
    p32 = prob.reshape(n, -1, k).float()
    t32 = target.reshape(n, -1, k).float()
    pos = p32 >= torch.tensor(threshold, dtype=torch.float32, device=p32.device)
    fg = t32 >= 0.5
    p, t = p32.double(), t32.double()
    out = torch.stack([(t * p).sum(1), t.sum(1), p.sum(1),
                       (pos & fg).sum(1).double(), (pos & ~fg).sum(1).double(), (~pos & fg).sum(1).double()], dim=-1)
    return out


def _np(stats) -> np.ndarray:
    if isinstance(stats, torch.Tensor):
        stats = stats.detach().cpu().numpy()
    a = np.asarray(stats, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != NSLOT:
        raise ValueError("case statistics must be [N][K][6], got %s" % (a.shape,))
    return a


def accumulate(stats, S: int, valid=None) -> Dict[str, np.ndarray]:
    """Additive accumulators of the hard metrics over the cases of ``stats`` (``valid``: an
    optional boolean mask over them): per class the pooled TP / FP / FN / TN and the sum of
    the per-case Dice, plus the case count.  Accumulators of disjoint case sets add."""
    a = _np(stats)
    if valid is not None:
        a = a[np.asarray(valid, dtype=bool)]
    tp, fp, fn = a[:, :, 3], a[:, :, 4], a[:, :, 5]
    den = 2.0 * tp + fp + fn
    cd = np.where(den > 0, 2.0 * tp / np.where(den > 0, den, 1.0), 1.0)
    return {"tp": tp.sum(0), "fp": fp.sum(0), "fn": fn.sum(0), "tn": (float(S) - tp - fp - fn).sum(0),
            "case_dice_sum": cd.sum(0), "cases": float(a.shape[0])}


def _ratio(num: np.ndarray, den: np.ndarray):
    return [float(n / d) if d > 0 else float("nan") for n, d in zip(num, den)]


def hard_metrics(acc: Dict[str, np.ndarray]) -> dict:
    """case_dice / sensitivity / specificity per class from :func:`accumulate` sums."""
    cases = float(acc["cases"])
    cd = [float(v / cases) if cases > 0 else float("nan") for v in acc["case_dice_sum"]]
    return {"case_dice": cd,
            "case_dice_mean": float(np.mean(cd)) if cd else float("nan"),
            "sensitivity": _ratio(acc["tp"], acc["tp"] + acc["fn"]),
            "specificity": _ratio(acc["tn"], acc["tn"] + acc["fp"]),
            "cases": int(cases)}


def soft_dice(stats) -> list:
    """Per-class soft Dice (smoothing 1) on the sums over the samples of ``stats``."""
    a = _np(stats)
    i, st, sp = a[:, :, 0].sum(0), a[:, :, 1].sum(0), a[:, :, 2].sum(0)
    return [float(v) for v in (2.0 * i + SMOOTH) / (st + sp + SMOOTH)]


def metrics_from_case_stats(stats, S: int, valid=None) -> dict:
    """``{"dice": [K], "case_dice": [K], "case_dice_mean", "sensitivity": [K],
    "specificity": [K], "cases"}`` of the (valid) cases of ``stats``."""
    a = _np(stats)
    if valid is not None:
        a = a[np.asarray(valid, dtype=bool)]
    m = hard_metrics(accumulate(a, S))
    m["dice"] = soft_dice(a)
    return m


# ---------------------------------------------------------------------------------------
# 95th-percentile Hausdorff distance (HD95)
#
# ``surf[n][k] = {mp, mt, q_lo, q_hi}`` of sample n and class k, on the sample's grid (H x W,
# or D x H x W; unit spacing, distances in voxels): with P = {p >= float32(thr)} and
# T = {t >= 0.5}, the surface of a mask is its voxels with a face neighbour (4 in 2D, 6 in
# 3D) outside the mask, a neighbour outside the grid counting as outside the mask
# (``A & ~binary_erosion(A)`` with scipy's defaults).  ``mp`` and ``mt`` are the surface sizes.
# Q is the multiset of squared distances from every surface voxel of P to the surface of T
# and the reverse, ``m = mp + mt``, ``r = 95 (m - 1)``, ``lo = r // 100``,
# ``hi = min(lo + 1, m - 1)``: ``q_lo`` and ``q_hi`` are the elements of rank lo and hi of
# sorted Q, or -1 when a surface is empty.  Then
# ``hd95 = sqrt(q_lo) + (r % 100) / 100 * (sqrt(q_hi) - sqrt(q_lo))``, which is
# ``numpy.percentile(hstack(d_PT, d_TP), 95)`` (the MedPy convention).  Both surfaces empty
# score 0.0; exactly one empty scores the grid diagonal ``sqrt(D^2 + H^2 + W^2)``, D = 1 in 2D.  The native executors produce the
# integers with the separable distance transform of ``csrc/kernels/surf_dist.h``;
# :func:`case_surface_torch` finds them from all pairs of surface voxels.

NSURF = 4
_PAIR_CHUNK = 1 << 22           # distances formed at a time by the all-pairs oracle


def _grid_of(shape) -> tuple:
    g = tuple(int(v) for v in shape)
    if len(g) == 3 and g[0] == 1:           # (a one-slice volume is a 2D grid)
        g = g[1:]
    if len(g) not in (2, 3):
        raise ValueError("a sample grid is (H, W) or (D, H, W), got %s" % (tuple(shape),))
    return g


def _surface(mask: torch.Tensor) -> torch.Tensor:
    """Voxels of the boolean ``mask`` (one sample's grid) with a face neighbour outside it."""
    inner = mask.clone()
    for ax in range(mask.dim()):
        pad = torch.zeros_like(mask.narrow(ax, 0, 1))
        inner &= torch.cat([pad, mask.narrow(ax, 0, mask.shape[ax] - 1)], dim=ax)
        inner &= torch.cat([mask.narrow(ax, 1, mask.shape[ax] - 1), pad], dim=ax)
    return mask & ~inner


def _directed(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """int64 [len(a)]: squared distance from every coordinate row of ``a`` to the nearest of ``b``."""
    out = torch.empty(a.shape[0], dtype=torch.int64, device=a.device)
    step = max(1, _PAIR_CHUNK // max(1, b.shape[0]))
    for i in range(0, a.shape[0], step):
        d = a[i:i + step, None, :] - b[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(dim=1).values
    return out


@torch.no_grad()
def case_surface_torch(prob: torch.Tensor, target: torch.Tensor, threshold: float = 0.5, grid=None) -> torch.Tensor:
    """int64 ``[N][K][4] = {mp, mt, q_lo, q_hi}`` from ``prob`` / ``target`` of shape
    ``[N, *grid, K]`` (or ``[N, S, K]`` with ``grid`` given): surface coordinates, all-pairs
    squared distances in int64 and a sort."""
    n, k = prob.shape[0], prob.shape[-1]
    grid = _grid_of(prob.shape[1:-1] if grid is None else grid)
    p32 = prob.reshape((n,) + grid + (k,)).float()
    t32 = target.reshape((n,) + grid + (k,)).float()
    pos = p32 >= torch.tensor(threshold, dtype=torch.float32, device=p32.device)
    fg = t32 >= 0.5
    out = torch.empty(n, k, NSURF, dtype=torch.int64)
    for i in range(n):
        for c in range(k):
            a = torch.nonzero(_surface(pos[i, ..., c])).long()
            b = torch.nonzero(_surface(fg[i, ..., c])).long()
            mp, mt = a.shape[0], b.shape[0]
            if mp == 0 or mt == 0:
                out[i, c] = torch.tensor([mp, mt, -1, -1])
                continue
            q = torch.sort(torch.cat([_directed(a, b), _directed(b, a)])).values
            m = mp + mt
            lo = 95 * (m - 1) // 100
            hi = min(lo + 1, m - 1)
            out[i, c] = torch.tensor([mp, mt, int(q[lo]), int(q[hi])])
    return out


def _np_surf(surf) -> np.ndarray:
    if isinstance(surf, torch.Tensor):
        surf = surf.detach().cpu().numpy()
    a = np.asarray(surf, dtype=np.int64)
    if a.ndim != 3 or a.shape[2] != NSURF:
        raise ValueError("case surface integers must be [N][K][4], got %s" % (a.shape,))
    return a


def hd95_from_surface(surf, grid) -> np.ndarray:
    """float64 ``[N][K]`` HD95 in voxels from ``{mp, mt, q_lo, q_hi}`` on ``grid`` = (H, W)
    or (D, H, W): 0.0 when both surfaces are empty, the grid diagonal when one is."""
    a = _np_surf(surf)
    mp, mt = a[:, :, 0], a[:, :, 1]
    both = (mp > 0) & (mt > 0)
    r = 95 * (mp + mt - 1)
    lo = np.sqrt(np.where(both, a[:, :, 2], 0).astype(np.float64))
    hi = np.sqrt(np.where(both, a[:, :, 3], 0).astype(np.float64))
    val = lo + (r % 100).astype(np.float64) / 100.0 * (hi - lo)
    g = tuple(int(v) for v in grid)
    if len(g) == 2:
        g = (1,) + g
    diag = math.sqrt(float(sum(v * v for v in g)))      # sqrt(D^2 + H^2 + W^2), D = 1 in 2D
    return np.where(both, val, np.where((mp == 0) & (mt == 0), 0.0, diag))


def accumulate_hd95(surf, grid, valid=None) -> Dict[str, np.ndarray]:
    """Additive accumulators of HD95 over the cases of ``surf`` (``valid``: an optional boolean
    mask over them): the per-class sum and the case count.  Disjoint case sets add."""
    h = hd95_from_surface(surf, grid)
    if valid is not None:
        h = h[np.asarray(valid, dtype=bool)]
    return {"hd95_sum": h.sum(0), "cases": float(h.shape[0])}


def hd95_metrics(acc: Dict[str, np.ndarray]) -> dict:
    """``{"hd95": [K], "hd95_mean"}``: the mean over cases per class (formed like
    ``case_dice``) and its mean over classes."""
    cases = float(acc["cases"])
    h = [float(v / cases) if cases > 0 else float("nan") for v in acc["hd95_sum"]]
    return {"hd95": h, "hd95_mean": float(np.mean(h)) if h else float("nan")}


def jsonable(o):
    """``o`` with every non-finite float replaced by ``None`` (JSON ``null``): strict JSON
    has no NaN, and an undefined ratio must not read as a number."""
    if isinstance(o, dict):
        return {k: jsonable(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [jsonable(v) for v in o]
    if isinstance(o, (float, np.floating)):
        return float(o) if math.isfinite(o) else None
    if isinstance(o, np.integer):
        return int(o)
    return o


def fmt(v: Optional[float]) -> str:
    return "nan" if v is None or not math.isfinite(v) else "%.4f" % v

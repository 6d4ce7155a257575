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

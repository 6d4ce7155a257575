"""Connected-component post-processing of thresholded probability maps: the definition.

``p`` fp32 ``[N, (D,) H, W, K]`` (channels-last), ``thr`` in (0, 1).  Per (sample, class) the
foreground is ``F = {p >= thr}``; two voxels of F are connected when they share a face (4
neighbours in 2D, 6 in 3D: the connectivity of the HD95 surface).  Diagonal contact does not
connect, the border does not wrap, samples and classes never connect.

* a component's label is the smallest linear index ``(z H + y) W + x`` it contains, its size
  its voxel count;
* the largest component has the maximal size; among equal sizes the smallest label wins;
* the policy ``(keep_largest, min_size)`` keeps a component when ``size >= min_size`` and, with
  ``keep_largest``, it is the largest one (nothing if that one is below ``min_size``);
* ``out = p`` outside F and on kept components, ``0.0`` on removed ones;
* ``info int32 [N][K][4] = {components, kept components, largest size (0: none), kept voxels}``.

``components_torch`` is the oracle of the HIP op (``csrc/kernels/components.h``) and what the
ATen backend runs; the kernel's output equals it under ``torch.equal``.
"""

from typing import Tuple

import torch


def parse_policy(s: str) -> Tuple[bool, int]:
    """(keep_largest, min_size) of a validated --eval_components string (``config.parse_components``)."""
    from ..config import parse_components
    return parse_components(s)


def describe(s: str) -> str:
    """'largest, min 20 voxels' for the start-up line."""
    largest, v = parse_policy(s)
    return ", ".join((["largest"] if largest else []) + (["min %d voxels" % v] if v else []))


def _planes(p: torch.Tensor, thr: float):
    """(F bool [N, K, D, H, W], (D, H, W)) of channels-last probabilities."""
    if p.dim() not in (4, 5):
        raise ValueError("components: probabilities [N, (D,) H, W, K] expected, got %s" % (tuple(p.shape),))
    if not 0.0 < thr < 1.0:
        raise ValueError("components: threshold strictly inside (0, 1)")
    q = p if p.dim() == 5 else p.unsqueeze(1)
    return (q >= thr).permute(0, 4, 1, 2, 3).contiguous(), tuple(q.shape[1:4])


def _labels(F: torch.Tensor) -> torch.Tensor:
    """int64 [N, K, D, H, W]: the smallest linear index of each voxel's component, -1 outside F.

    Min-label propagation to the fixpoint (label equivalence): a round takes every voxel's
    minimum m over its face neighbours in F, lowers the voxel's label and the label of its
    label to m, and then replaces labels by their labels until nothing changes.  A label
    always names a voxel of the same component and is never above the voxel's own index, so
    at the fixpoint, where neighbours agree, every component carries its smallest index."""
    N, K, D, H, W = F.shape
    S = D * H * W
    idx = torch.arange(S, device=F.device).view(1, 1, D, H, W).expand(N, K, D, H, W)
    lab = torch.where(F, idx, torch.full_like(idx, S)).contiguous()       # (S: outside F, the pad slot's index)
    pad = lab.new_full((N, K, 1), S)
    while True:
        m = lab.clone()
        for ax, L in ((2, D), (3, H), (4, W)):
            if L == 1:
                continue
            lo, hi = lab.narrow(ax, 0, L - 1), lab.narrow(ax, 1, L - 1)   # (S outside F: never the minimum)
            ml, mh = m.narrow(ax, 0, L - 1), m.narrow(ax, 1, L - 1)
            ml.copy_(torch.minimum(ml, hi))
            mh.copy_(torch.minimum(mh, lo))
        m = torch.where(F, m, lab).view(N, K, S)
        old = torch.cat([lab.view(N, K, S), pad], dim=2)
        new = old.scatter_reduce(2, old[..., :S], m, "amin")              # the label's label
        new[..., :S] = torch.minimum(new[..., :S], m)
        new[..., S] = S
        while True:
            jump = new.gather(2, new)
            if torch.equal(jump, new):
                break
            new = jump
        if torch.equal(new, old):
            break
        lab = new[..., :S].reshape(N, K, D, H, W)
    return torch.where(F, lab, torch.full_like(lab, -1))


def labels_torch(p: torch.Tensor, thr: float) -> torch.Tensor:
    """int64 label map ``[N, K, (D,) H, W]`` of ``{p >= thr}``: each voxel's component label
    (the component's smallest linear index), -1 outside the foreground."""
    F, _ = _planes(p, float(thr))
    lab = _labels(F)
    return lab if p.dim() == 5 else lab[:, :, 0]


def components_torch(p: torch.Tensor, thr: float, keep_largest: bool, min_size: int):
    """(out fp32 like p, info int32 [N][K][4]) of the policy (keep_largest, min_size)."""
    min_size = int(min_size)
    if min_size < 0:
        raise ValueError("components: min_size >= 0")
    p = p.float()
    F, (D, H, W) = _planes(p, float(thr))
    N, K = F.shape[:2]
    S = D * H * W
    lab = _labels(F).view(N, K, S)
    Ff = F.view(N, K, S)
    size = torch.zeros(N, K, S + 1, dtype=torch.int64, device=p.device)
    size.scatter_add_(2, torch.where(Ff, lab, torch.full_like(lab, S)), Ff.long())
    size = size[..., :S]                                   # size[n, k, label] (0 where no component starts)
    comps = (size > 0).sum(dim=2)
    # the largest: maximal size, the smallest label among equals (argmax of size * (S + 1) - label)
    key = size * (S + 1) + (S - torch.arange(S, device=p.device))
    key = torch.where(size > 0, key, torch.zeros_like(key))
    best = key.argmax(dim=2)
    largest = size.gather(2, best.unsqueeze(2)).squeeze(2)
    kept = (size > 0) & (size >= min_size)
    if keep_largest:
        only = torch.zeros_like(kept)
        only.scatter_(2, best.unsqueeze(2), torch.ones_like(best, dtype=torch.bool).unsqueeze(2))
        kept = kept & only
    info = torch.stack([comps, kept.sum(dim=2), largest, (size * kept).sum(dim=2)], dim=2).to(torch.int32)
    kept_vox = torch.cat([kept, kept.new_zeros(N, K, 1)], dim=2).gather(
        2, torch.where(Ff, lab, torch.full_like(lab, S)))
    drop = (Ff & ~kept_vox).view(N, K, D, H, W).permute(0, 2, 3, 4, 1)
    if p.dim() == 4:
        drop = drop[:, 0]
    return torch.where(drop, torch.zeros_like(p), p), info

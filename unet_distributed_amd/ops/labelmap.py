"""Label maps from probability maps: the definition.

``prob`` fp32 ``[N, (D,) H, W, K]`` (channels-last, K = 1..4), ``threshold`` in (0, 1).  Per
voxel ``on_k = prob_k >= threshold`` -- both sides fp32, the comparison of ``components`` and
``seg_stats``; NaN is never on -- and the slot ``m`` is

* ``rule = "nested"``: the number of leading channels that are on, the largest m with
  ``on_0 .. on_{m-1}`` all true (a channel that is on above one that is off does not count);
* ``rule = "argmax"``: 0 when no channel is on, else ``1 + k*`` with ``k*`` the on channel of the
  greatest probability, the lowest index among equals (a sequential scan with a strict ``>``
  from ``-inf``).

``label = values[m]`` with ``values[0] = 0`` and ``values[1..K]`` in 1..255; ``counts[n][m]`` is
the number of source voxels of image n in slot m (the slots of an image sum to ``D H W``).

Source voxel ``(d, h, w)`` lands at ``(d + od, h + oh, w + ow)`` of the destination
``out_shape``; every destination voxel outside that box is 0.

``labelmap_torch`` is the oracle of the HIP op (``csrc/kernels/labelmap.h``) and what the ATen
backend runs; the kernel's output equals it under ``torch.equal``.
"""

from typing import Optional, Sequence, Tuple

import torch

RULES = ("nested", "argmax")
# --mode 5 trains whole tumour, core, enhancing (`datasets.select_masks`): edema outside the core,
# necrotic / non-enhancing core, enhancing -- its inverse up to BraTS labels 1 and 3, which the
# regions do not separate
MODE5_VALUES = (2, 1, 4)


def default_values(K: int, mode: Optional[int] = None) -> Tuple[int, ...]:
    return MODE5_VALUES if K == 3 and mode == 5 else tuple(range(1, K + 1))


def parse_labels(spec: str, K: int, mode: Optional[int] = None) -> Tuple[str, Tuple[int, ...]]:
    """(rule, values[1..K]) of the public spelling ``"<rule>[:v1,v2,..]"``; "" is nested with the
    default values (``2, 1, 4`` for K = 3 in mode 5, else ``1..K``).  An unknown rule, a wrong
    count of values, a value outside 1..255 or a repeated value is a SystemExit that names it."""
    s = str(spec).strip()
    if not s:
        return "nested", default_values(K, mode)
    rule, _, tail = s.partition(":")
    rule = rule.strip()
    if rule not in RULES:
        raise SystemExit("--labels: unknown rule %r (choose from %s)" % (rule, ", ".join(RULES)))
    if ":" not in s:
        return rule, default_values(K, mode)
    items = [t.strip() for t in tail.split(",")]
    if len(items) != K:
        raise SystemExit("--labels: %d values for %d output channels, got %r" % (K, K, tail))
    values = []
    for t in items:
        if not t.isdigit() or not 1 <= int(t) <= 255:
            raise SystemExit("--labels: a value is an integer in 1..255, got %r" % t)
        if int(t) in values:
            raise SystemExit("--labels: value %r is listed twice" % t)
        values.append(int(t))
    return rule, tuple(values)


def describe(rule: str, values: Sequence[int]) -> str:
    """'nested, values 2,1,4' for the start-up line."""
    return "%s, values %s" % (rule, ",".join(str(int(v)) for v in values))


def pack_values(values: Sequence[int]) -> int:
    """values[1..K] as the op's one integer: values[m] in byte m - 1."""
    return sum(int(v) << (8 * i) for i, v in enumerate(values))


def check_values(values: Sequence[int], K: int) -> Tuple[int, ...]:
    values = tuple(int(v) for v in values)
    if len(values) != K or any(not 1 <= v <= 255 for v in values):
        raise ValueError("labelmap: %d values in 1..255 expected, got %r" % (K, values))
    return values


def box(src: Sequence[int], out_shape: Optional[Sequence[int]], offset: Sequence[int]):
    """((Do, Ho, Wo), (od, oh, ow)) of a source (D, H, W); ValueError when the box does not fit."""
    src = tuple(int(v) for v in src)
    off = tuple(int(v) for v in offset)
    dst = src if out_shape is None else tuple(int(v) for v in out_shape)
    if src[0] == 1:                           # (a 2D source: pairs (H, W) are taken as (1, H, W) / (0, oh, ow))
        dst = (1,) + dst if len(dst) == 2 else dst
        off = (0,) + off if len(off) == 2 else off
    if len(dst) != 3 or len(off) != 3:
        raise ValueError("labelmap: out_shape and offset are (D, H, W) triples, got %r and %r" % (dst, off))
    if any(o < 0 or s < 1 or o + s > d for s, d, o in zip(src, dst, off)):
        raise ValueError("labelmap: the source %r at offset %r does not fit the destination %r" % (src, off, dst))
    return dst, off


def geometry(prob: torch.Tensor, out_shape, offset):
    """(N, (D, H, W), K, (Do, Ho, Wo), (od, oh, ow)) of probabilities [N, (D,) H, W, K]."""
    if prob.dim() not in (4, 5):
        raise ValueError("labelmap: probabilities [N, (D,) H, W, K] expected, got %s" % (tuple(prob.shape),))
    src = tuple(prob.shape[1:4]) if prob.dim() == 5 else (1,) + tuple(prob.shape[1:3])
    dst, off = box(src, out_shape, offset)
    if prob.dim() == 4 and dst[0] != 1:
        raise ValueError("labelmap: a 2D map has a destination of depth 1, got %r" % (dst,))
    return prob.shape[0], src, prob.shape[-1], dst, off


def slots_torch(prob: torch.Tensor, threshold: float, rule: str) -> torch.Tensor:
    """int64 slot m of every voxel of fp32 probabilities ``[..., K]``."""
    if rule not in RULES:
        raise ValueError("labelmap: rule must be one of %s, got %r" % (", ".join(RULES), rule))
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError("labelmap: threshold strictly inside (0, 1)")
    K = prob.shape[-1]
    if not 1 <= K <= 4:
        raise ValueError("labelmap: 1..4 classes, got %d" % K)
    prob = prob.float()
    on = prob >= torch.tensor(float(threshold), dtype=torch.float32, device=prob.device)
    m = torch.zeros(prob.shape[:-1], dtype=torch.int64, device=prob.device)
    if rule == "nested":                      # (a loop over K <= 4 channels: elementwise ops only, any size)
        run = torch.ones_like(on[..., 0])
        for k in range(K):
            run = run & on[..., k]
            m += run
        return m
    best = torch.full(prob.shape[:-1], float("-inf"), dtype=torch.float32, device=prob.device)
    for k in range(K):
        take = on[..., k] & (prob[..., k] > best)
        best = torch.where(take, prob[..., k], best)
        m = torch.where(take, torch.full_like(m, k + 1), m)
    return m


def labelmap_torch(prob: torch.Tensor, threshold: float, rule: str, values: Sequence[int],
                   out_shape: Optional[Sequence[int]] = None, offset: Sequence[int] = (0, 0, 0)):
    """(labels uint8 ``[N, (Do,) Ho, Wo]``, counts int64 ``[N][K + 1]``) of fp32 probabilities
    ``[N, (D,) H, W, K]``.  `out_shape` / `offset` are (D, H, W) triples (D = 1 and od = 0 in 2D);
    ``out_shape=None`` is the source shape at zero offset."""
    N, _, K, dst, off = geometry(prob, out_shape, offset)
    values = check_values(values, K)
    q = prob if prob.dim() == 5 else prob.unsqueeze(1)
    m = slots_torch(q, threshold, rule)
    table = torch.tensor((0,) + values, dtype=torch.uint8, device=prob.device)
    counts = torch.zeros(N, K + 1, dtype=torch.int64, device=prob.device)
    counts.scatter_add_(1, m.reshape(N, -1), torch.ones_like(m).reshape(N, -1))
    out = torch.zeros((N,) + dst, dtype=torch.uint8, device=prob.device)
    D, H, W = q.shape[1:4]
    out[:, off[0]:off[0] + D, off[1]:off[1] + H, off[2]:off[2] + W] = table[m]
    return (out if prob.dim() == 5 else out[:, 0]), counts

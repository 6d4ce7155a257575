"""Static validation of the native executor's launch plans (no GPU needed).

The planner (`runtime/native_engine.py`) decides a dozen cross-layer fusions whose
legality depends on the config (norm x decoder x dims x image size).  A wrong decision
shows up either as a launch whose parameters no built kernel accepts, or as a kernel
reading a buffer nothing wrote in that step (silently stale data).  This module checks
both on a dry-run plan:

* **dispatch** -- every op of the training and evaluation plans is run through its
  launcher under dry dispatch (`Plan.check_dispatch`, conv_params.h `dry_dispatch`): the
  launcher resolves its template instantiation / tile / epilogue and reports whether a
  kernel exists, without launching;
* **def-use** -- the executor records each op's parameters (`RecordingPlan`); every
  pointer an op reads must lie in a buffer that an EARLIER op of the same plan wrote, or
  in a step input (the batch, the weights, the running statistics, workspaces); pointers
  into no known buffer, and buffers the planner dropped (never formed), are errors;
* **coverage** -- every parameter's gradient (per variable of the flat buffer) is
  written by the training plan.

The reference has no such machinery (its graph is TF's, `test_dist.py:183-298`); this is
the static-graph executor's equivalent of TF's graph validation.
"""

from typing import Dict, List, NamedTuple, Tuple

import torch

_HG = ("hg_prob", "hg_t", "hg_sums", "hg_w", "hg_bits", "hg_gscale", "hg_fa", "hg_fc")
CONV_READS = ("src1", "src2", "wgt", "bias", "mask1", "mask2", "route_gy", "nz", "na", "nc", "xa", "xb", "xc", "xz",
              "ut_x", "ut_w", "ut_b", "head_w", "head_b", "head_t", "fw_x") + _HG
CONV_WRITES = ("dst1", "dst2", "stats", "relu_bits", "pool_dst", "head_logit", "head_ws", "xout", "fw_slab",
               "fw_bias_slab")
WGRAD_READS = ("a1", "a2", "b", "xa", "xb", "xc", "xz") + _HG
WGRAD_WRITES = ("slab", "bias_slab")


class GatherRow(NamedTuple):
    """Layout of one batch gather's generic op (bindings.cpp): ptrs = x_all, y_all, idx, `slots`,
    xb, tb; ints = B, (Ds, Hs, Ws when `patch` is 4,) D, H, W, Cin, Cpad, K (, s for the ops with a field)."""
    slots: Tuple[str, ...]      # the op's own pointers, in order
    nints: int
    patch: int                  # index of the patch's D in ints

    @property
    def xb(self) -> int:        # index of xb in ptrs; tb follows it
        return 3 + len(self.slots)


GATHER_OPS = {
    "gather_batch_aug": GatherRow(("code", "affine"), 7, 1),
    "gather_batch_crop": GatherRow(("origin", "code", "affine"), 10, 4),
    "gather_batch_warp": GatherRow(("origin", "code", "mat", "affine"), 10, 4),
    "gather_batch_elastic": GatherRow(("origin", "code", "mat", "affine", "field"), 11, 4),
    "gather_batch_warp3": GatherRow(("origin", "code", "mat", "affine", "field"), 11, 4),
}


def _gather_row(kind: str):
    """The row of generic op `kind` (16-bit or "f32_") in GATHER_OPS, or None."""
    return GATHER_OPS.get(kind[4:] if kind.startswith("f32_") else kind)


def _sel(p, idx):
    return [p[i] for i in idx if i < len(p)]


def _conv_write_spans(d, stat_tiles=None) -> List[Tuple[int, int]]:
    """(pointer, bytes) of the writes of 16-bit conv dict `d` whose extent follows from its
    shape (the executor's offset arithmetic -- batch chunks, tail halves, channel splits,
    slab rows -- must keep each inside its buffer)."""
    g = d.get
    N, OD, OH, OW = g("N", 1), g("OD", 1) or 1, g("OH", 1), g("OW", 1)
    M = N * OD * OH * OW
    Cout = g("Cout", 0)
    D1 = g("D1") or Cout
    out = []
    if g("shuffle"):
        out.append((g("dst1"), M * Cout * 2))
    else:
        out.append((g("dst1"), M * D1 * 2))
        if g("dst2"):
            out.append((g("dst2"), M * (Cout - D1) * 2))
    if g("relu_bits"):
        out.append((g("relu_bits"), M * Cout // 8))
    if g("head_logit"):
        out.append((g("head_logit"), M * 4))
    if g("head_ws"):
        out.append((g("head_ws"), g("head_ws_rows", 0) * 100 * 4))
    if g("pool_dst"):
        out.append((g("pool_dst"), M // 4 * Cout * 2))
        out.append((g("pool_code"), M // 4 * Cout // 8 * 4))
    if g("xout"):
        out.append((g("xout"), M * g("C1", 0) * 2))
    if g("fw_x"):
        rows = g("fw_split_lo", 0) + g("fw_nsplit", 0)
        out.append((g("fw_slab"), rows * 9 * g("fw_Cx", 0) * g("C1", 0) * 4))
        out.append((g("fw_bias_slab"), rows * g("C1", 0) * 4))
    if g("stats") and stat_tiles is not None:
        rows = stat_tiles(d)
        if rows:
            out.append((g("stats"), rows * 2 * Cout * 4))
    return [(p, n) for p, n in out if p]


def _generic_write_spans(kind: str, p: List[int], ints: List[int]) -> List[Tuple[int, int]]:
    """(pointer, bytes) of the writes of the streaming norm passes (N, P, C in ints) and
    the head dY pass (P, C)."""
    if kind in ("norm_apply", "norm_bwd_apply") and len(p) > 5 and len(ints) >= 3:
        return [(p[5], ints[0] * ints[1] * ints[2] * 2)]
    if kind == "head_dy" and len(p) > 5 and len(ints) >= 2:
        return [(p[5], ints[0] * ints[1] * 2)]
    # standalone head (P, C [, K classes] in ints): K-wide probabilities / Mask gradients and
    # the per-block partial rows (head_blocks(P) = min(ceil(P / 256), 1024) rows)
    if kind in ("head_fwd", "head_bwd") and len(ints) >= 2:
        P, C = ints[0], ints[1]
        K = ints[2] if len(ints) > 2 else 1
        nb = max(1, min(-(-P // 256), 1024))
        if kind == "head_fwd" and len(p) > 6:
            # (loss partials: 4 floats per block; the K-class forward runs up to 2 nb blocks)
            return [(p[4], P * K * 4), (p[5], (nb if K == 1 else 2 * nb) * 4 * 4), (p[6], 4 * 4)]
        if kind == "head_bwd" and len(p) > 8:
            return [(q, n) for q, n in ((p[5], P * C * 2), (p[6], nb * (C + 1) * K * 4), (p[7], C * K * 4),
                                        (p[8], K * 4)) if q]
    # per-(sample, class) statistics (N, S, K in ints): N K 6 floats of stats and one row of
    # 6 K floats per (sample, chunk) of the partial buffer
    if kind in ("seg_stats", "f32_seg_stats") and len(p) > 2 and len(ints) >= 3:
        N, S, K = ints[0], ints[1], ints[2]
        out = [(p[2], N * K * 6 * 4)]
        chunks = seg_stats_chunks(N, S, K)
        if len(p) > 3 and p[3] and chunks > 1:
            out.append((p[3], N * chunks * 6 * K * 4))
        return out
    # surface distances (N, D, H, W, K in ints): N K 4 ints of output and the field scratch
    if kind in ("surf_dist", "f32_surf_dist") and len(p) > 3 and len(ints) >= 5:
        N, D, H, W, K = ints[:5]
        return [(p[2], N * K * 4 * 4), (p[3], surf_dist_scratch(N, D, H, W, K))]
    # component filter (N, D, H, W, K in ints): the filtered map, N K 4 ints of info and the scratch
    if kind == "components" and len(p) > 3 and len(ints) >= 5:
        N, D, H, W, K = ints[:5]
        return [(p[1], N * D * H * W * K * 4), (p[2], N * K * 4 * 4), (p[3], components_scratch(N, D, H, W, K))]
    # label map (N, D, H, W, K, Do, Ho, Wo in ints): the whole uint8 destination and N 5 ints of counts
    if kind == "labelmap" and len(p) > 2 and len(ints) >= 8:
        return [(p[1], ints[0] * ints[5] * ints[6] * ints[7]), (p[2], ints[0] * 5 * 4)]
    # the batch gathers: the padded input and the target of the patch's size, 16-bit or fp32 (f32_)
    g = _gather_row(kind)
    if g and len(p) > g.xb + 1 and len(ints) >= g.nints:
        B, (D, H, W, _, cpad, K) = ints[0], ints[g.patch:g.patch + 6]
        eb = 4 if kind.startswith("f32") else 2
        return [(p[g.xb], B * D * H * W * cpad * eb), (p[g.xb + 1], B * D * H * W * K * eb)]
    # test-time augmentation: the fp32 accumulator (N, D, H, W, K in ints); the finish (total
    # elements in ints) rewrites prob and writes one row of 4 floats per block and the 4 sums
    if kind == "tta_acc" and len(p) > 1 and len(ints) >= 5:
        N, D, H, W, K = ints[:5]
        return [(p[1], N * D * H * W * K * 4)]
    if kind in ("tta_finish", "f32_tta_finish") and len(p) > 4 and len(ints) >= 1:
        return [(p[0], ints[0] * 4), (p[3], tta_finish_blocks(ints[0]) * 4 * 4), (p[4], 4 * 4)]
    # sliding window (N, D, H, W, C | K, Td, Th, Tw, sd, sh, sw, B, t0, nt in ints): the staging
    # batch; the accumulator up to the end of the last image the batch touches; the whole accumulator
    if kind == "sw_extract" and len(p) > 1 and len(ints) >= 14:
        return [(p[1], ints[11] * ints[5] * ints[6] * ints[7] * ints[4] * 4)]
    if kind == "sw_blend" and len(p) > 2 and len(ints) >= 14:
        from ..ops.sliding import tiles_per_image
        tpi = tiles_per_image(ints[1:4], ints[5:8], ints[8:11])
        last = (ints[12] + ints[13] - 1) // tpi
        return [(p[2], (last + 1) * ints[1] * ints[2] * ints[3] * ints[4] * 4)]
    if kind == "sw_finish" and len(p) > 1 and len(ints) >= 5:
        N, D, H, W, K = ints[:5]
        return [(p[0], N * D * H * W * K * 4)]
    return []


def tta_finish_blocks(total: int) -> int:
    """Blocks of a tta_finish launch (mirrors csrc/kernels/tta.hip)."""
    return max(1, min(-(-(total // 4) // 256), 1024))


def seg_stats_chunks(N: int, S: int, K: int) -> int:
    """Chunks per sample of a seg_stats launch (mirrors csrc/kernels/seg_stats.hip)."""
    it = 256 * (3 if K == 3 else 4)
    iters = -(-(S // 8 * K) // it)
    chunks = max(1, min(-(-1024 // N), 256, iters))
    per = -(-iters // chunks)
    return -(-iters // per)


def surf_dist_scratch(N: int, D: int, H: int, W: int, K: int) -> int:
    """Scratch bytes of a surf_dist launch over N samples: int32 fields [N][K][2][S]
    (mirrors csrc/kernels/surf_dist.hip)."""
    return N * K * 2 * D * H * W * 4


def components_scratch(N: int, D: int, H: int, W: int, K: int) -> int:
    """Scratch bytes of a components launch over N samples: int32 label and size planes
    [N][K][S], sel [N][K] and the selection's parts [N][K][P][5], P = ceil(S / 16384), rounded up
    to 16 (mirrors csrc/kernels/f32_components.hip)."""
    S = D * H * W
    return (N * K * (2 * S + 1 + 5 * (-(-S // 16384))) * 4 + 15) // 16 * 16


def _generic_rw(kind: str, p: List[int], ints: List[int]) -> Tuple[List[int], List[int]]:
    """(read pointers, written pointers) of one generic op (layouts: bindings.cpp)."""
    if kind == "ups_fwd":
        return _sel(p, [0]), _sel(p, [1])
    if kind == "ups_bwd":
        return _sel(p, [0, 1]), _sel(p, [2])
    if kind == "pool_fwd":
        return _sel(p, [0]), _sel(p, [1, 2])
    if kind == "pool_bwd":
        return (_sel(p, [1, 2, 4]) if len(p) > 4 and p[4] else _sel(p, [0, 1, 2])), _sel(p, [3])
    if kind == "pool_bwd_norm":
        return _sel(p, [0, 1, 2, 3]), _sel(p, [4, 5])
    if kind == "norm_pool":
        return _sel(p, [0, 1, 2]), _sel(p, [3, 4, 5])
    if kind == "norm_apply" or kind == "norm_bwd_apply":
        return _sel(p, [0, 1, 2, 3, 4]), _sel(p, [5])
    if kind == "norm_rows":
        return _sel(p, [0, 1]), _sel(p, [2])
    if kind == "bn_stats":
        mode = ints[2]
        if mode == 0:
            return _sel(p, [0, 1, 2, 3, 4, 14]), _sel(p, [3, 4, 5, 6, 7, 8, 14])
        if mode == 1:
            return _sel(p, [0, 1, 2, 5, 6, 14]), _sel(p, [9, 10, 11, 12, 13, 14])
        return _sel(p, [1, 2, 3, 4]), _sel(p, [5, 6, 7, 8])
    if kind == "gn_stats":
        if ints[5] == 0:
            return _sel(p, [0, 1, 2]), _sel(p, [3, 4, 5, 6, 12])
        return _sel(p, [0, 1, 3, 4, 12]), _sel(p, [7, 8, 9, 10, 11, 12])
    if kind == "head_finish":
        return _sel(p, [0, 1]), _sel(p, [0, 2, 3])
    if kind == "head_fwd":
        return _sel(p, [0, 1, 2, 3]), _sel(p, [4, 5, 6])
    if kind == "head_wsum_grad":
        return _sel(p, [0, 1, 4]), _sel(p, [2, 3])
    if kind == "head_dy":
        return _sel(p, [0, 1, 2, 3, 4, 6]), _sel(p, [5])
    if kind == "head_bwd":
        return _sel(p, [0, 1, 2, 3, 4, 9]), _sel(p, [5, 6, 7, 8])
    if kind == "norm_head":
        return _sel(p, [0, 1, 2, 3, 4]), _sel(p, [5, 6])
    if kind == "norm_head_loss":
        return _sel(p, [0, 1, 2, 3, 4, 5]), _sel(p, [6, 7, 8, 9])
    if kind == "head_norm_coef":
        return _sel(p, [0, 1, 2, 3, 4, 8]), _sel(p, [5, 6, 7])
    if kind == "head_norm_bwd":
        return _sel(p, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]), _sel(p, [10])
    if kind == "colsum":
        return _sel(p, [0]), _sel(p, [1])
    if kind in ("seg_stats", "f32_seg_stats"):
        return _sel(p, [0, 1]), _sel(p, [2, 3])
    if kind in ("surf_dist", "f32_surf_dist"):
        return _sel(p, [0, 1]), _sel(p, [2, 3])
    if kind == "components":
        return _sel(p, [0]), _sel(p, [1, 2, 3])
    if kind == "labelmap":
        return _sel(p, [0]), _sel(p, [1, 2])
    g = _gather_row(kind)
    if g:                                # (a null origin, code, matrix or affine is not read)
        return [q for q in p[:g.xb] if q], _sel(p, [g.xb, g.xb + 1])
    if kind == "tta_acc":                # (write mode reads no element of the accumulator)
        return _sel(p, [0, 1] if len(ints) > 6 and ints[6] else [0]), _sel(p, [1])
    if kind in ("tta_finish", "f32_tta_finish"):
        return _sel(p, [0, 1, 2]), _sel(p, [0, 3, 4])
    if kind == "sw_extract":
        return _sel(p, [0]), _sel(p, [1])
    if kind == "sw_blend":
        return _sel(p, [0, 1, 2]), _sel(p, [2])
    if kind == "sw_finish":
        return _sel(p, [0, 1]), _sel(p, [0])
    if kind == "tconv_compose":
        return _sel(p, [0, 1]), _sel(p, [2])
    if kind == "tconv_chain":
        return _sel(p, [0, 1, 2, 5, 6, 7]), _sel(p, [3, 4, 8])
    if kind == "wgrad_reduce":
        return _sel(p, [0]), _sel(p, [1, 2])
    if kind in ("f32_pool_fwd", "f32_ups_fwd", "f32_transpose"):
        return _sel(p, [0]), _sel(p, [1])
    if kind == "f32_pool_bwd":
        return _sel(p, [0, 1, 2]), _sel(p, [3])
    if kind == "f32_ups_bwd":
        return _sel(p, [0, 1]), _sel(p, [2])
    if kind == "f32_head_fwd":
        return _sel(p, [0, 1, 2, 3]), _sel(p, [4, 5, 6])
    if kind == "f32_head_bwd":
        return _sel(p, [0, 1, 2, 3, 4]), _sel(p, [5, 6, 7, 8])
    if kind == "f32_colsum":
        return _sel(p, [0]), _sel(p, [1, 2])
    if kind == "multi_reduce":
        return _sel(p, [0]), []          # slab / out pointers: the op's annotation (RecordingPlan.annotate)
    raise KeyError("plan_check: no read/write layout for generic op %r" % kind)


class RecordingPlan:
    """A native `_C.Plan` that also keeps each op's parameters for `check_plan`."""

    def __init__(self, plan, stat_tiles=None):
        self._plan = plan
        self._stat_tiles = stat_tiles        # conv dict -> statistics rows (extent of `stats`)
        self.ops: List[dict] = []

    def add_conv_fwd(self, d):
        i = self._plan.add_conv_fwd(d)
        reads = [d.get(k) for k in CONV_READS]
        writes = [d.get(k) for k in CONV_WRITES]
        (reads if d.get("route_gy") else writes).append(d.get("pool_code"))
        self.ops.append(dict(name=d.get("name", "conv_fwd"), reads=reads, writes=writes,
                             spans=_conv_write_spans(d, self._stat_tiles)))
        return i

    def add_wgrad(self, d):
        i = self._plan.add_wgrad(d)
        self.ops.append(dict(name=d.get("name", "wgrad"), reads=[d.get(k) for k in WGRAD_READS],
                             writes=[d.get(k) for k in WGRAD_WRITES]))
        return i

    def add_f32_conv(self, d):
        i = self._plan.add_f32_conv(d)
        self.ops.append(dict(name=d.get("name", "f32_conv"), reads=[d.get(k) for k in ("src1", "src2", "wgt", "bias",
                                                                                        "mask1")],
                             writes=[d.get("dst1")]))
        return i

    def add_f32_wgrad(self, d):
        i = self._plan.add_f32_wgrad(d)
        self.ops.append(dict(name=d.get("name", "f32_wgrad"), reads=[d.get(k) for k in ("a1", "a2", "b")],
                             writes=[d.get("slab")]))
        return i

    def add_generic(self, kind, ptrs, ints, floats, name=""):
        i = self._plan.add_generic(kind, ptrs, ints, floats, name)
        r, w = _generic_rw(kind, list(ptrs), list(ints))
        self.ops.append(dict(name=name or kind, reads=r, writes=w,
                             spans=_generic_write_spans(kind, list(ptrs), list(ints))))
        return i

    def annotate(self, reads=(), writes=()):
        """Extra pointers of the last op (e.g. the slabs / outputs of a multi_reduce job table)."""
        self.ops[-1]["reads"] += list(reads)
        self.ops[-1]["writes"] += list(writes)

    def __getattr__(self, k):
        return getattr(self._plan, k)


class _Regions:
    def __init__(self):
        self.spans: List[Tuple[int, int, str]] = []

    def add(self, name, t):
        if isinstance(t, torch.Tensor) and t.numel() > 0:
            a = int(t.data_ptr())
            self.spans.append((a, a + t.numel() * t.element_size(), name))

    def find(self, ptr):
        s = self.find_span(ptr)
        return None if s is None else s[2]

    def find_span(self, ptr):
        best = None
        for a, b, n in self.spans:
            if a <= ptr < b and (best is None or b - a < best[1] - best[0]):
                best = (a, b, n)
        return best


def engine_regions(e) -> Tuple[_Regions, set]:
    """Named buffers of executor `e` and the subset that are step inputs."""
    R = _Regions()
    inputs = set()
    for k, t in e.bufs.items():
        R.add(k, t)
    inputs.add("x")
    for k, t in getattr(e, "relu_bits", {}).items():
        R.add("bits:" + k, t)
    for k, t in getattr(e, "pool_codes", {}).items():
        R.add("code:" + k, t)
    for k, t in getattr(e, "wcopy", {}).items():          # fp32 executor: per-step weight layouts
        R.add("wcopy:" + k, t)
    for i, t in enumerate(getattr(e, "_keep", [])):         # fp32 executor: slabs / reduction stages
        R.add("keep%d" % i, t)
    R.add("colsum_part", getattr(e, "_colsum_part", None))
    for k, t in getattr(e, "_stat_bufs", {}).items():
        R.add("stat:" + k, t)
        if k.startswith("w"):                    # bn/gn_stats workspaces (self-contained)
            inputs.add("stat:" + k)
    for k in ("prob", "target", "sums", "head_partial", "head_ws", "slab", "bias_slab", "red_stage", "arena",
              "loss_scale_dev", "_no_dy", "case_stats_buf", "case_stats_partial",
              "case_surface_buf", "case_surface_scratch", "tta_acc_buf", "tta_partial",
              "sw_src", "sw_x", "sw_w", "sw_acc", "sw_wsum", "prob_pp", "components_info", "components_scratch"):
        R.add(k, getattr(e, k, None))
    inputs |= {"target", "arena", "loss_scale_dev", "_no_dy"}
    for k, t in getattr(e, "state", {}).items():
        R.add("state:" + k, t)
        inputs.add("state:" + k)
    for i, t in enumerate(getattr(e, "_job_tables", [])):
        R.add("jobs%d" % i, t)
        inputs.add("jobs%d" % i)
    for tn, tf in getattr(e, "tconv_fused", {}).items():
        for k in ("wg", "hs", "bs"):
            R.add("tf:%s:%s" % (tn, k), tf[k])
        if "wa" in tf:
            R.add("tf:%s:skg" % tn, tf["wa"]["skg"])
    for k, t in getattr(e, "_dropped", {}).items():
        R.add("dropped:" + k, t)
    f = e.flat
    for name, shape, off, n in f.entries:
        R.add("master:" + name, f.view(f.master, name))
        R.add("grad:" + name, f.view(f.grad, name))
        inputs.add("master:" + name)
    return R, inputs


def check_plan(e, plan, train: bool, extra_inputs=()) -> List[str]:
    """Errors of one recorded plan of executor `e` (empty list: valid).  extra_inputs: named
    buffers an earlier plan leaves behind for this one."""
    errs = []
    for i, name, err in plan.check_dispatch(0, plan.size()):
        errs.append("op %d %s: no kernel (%s)" % (i, name, err))
    R, inputs = engine_regions(e)
    inputs |= set(extra_inputs)
    written = set()
    for i, op in enumerate(plan.ops):
        for p in op["reads"]:
            if not p:
                continue
            r = R.find(int(p))
            if r is None:
                errs.append("op %d %s: reads unknown pointer 0x%x" % (i, op["name"], p))
            elif r.startswith("dropped:"):
                errs.append("op %d %s: reads %s, which the planner never forms" % (i, op["name"], r[8:]))
            elif r not in written and r not in inputs:
                errs.append("op %d %s: reads %s before any op writes it" % (i, op["name"], r))
        for p in op["writes"]:
            if not p:
                continue
            r = R.find(int(p))
            if r is None or r.startswith("dropped:") or r.startswith("master:"):
                errs.append("op %d %s: writes %s" % (i, op["name"], r or "unknown pointer 0x%x" % p))
            else:
                written.add(r)
        for p, n in op.get("spans", ()):
            sp = R.find_span(int(p))
            if sp is not None and int(p) + n > sp[1]:
                errs.append("op %d %s: writes %d bytes at %s+%d, past its end (%d bytes)"
                            % (i, op["name"], n, sp[2], int(p) - sp[0], sp[1] - sp[0]))
    if train:
        for name, shape, off, n in e.flat.entries:
            if "grad:" + name not in written:
                errs.append("no op writes the gradient of %s" % name)
    return errs


def check_engine(e) -> Dict[str, List[str]]:
    """{'train': errors, 'eval': errors} of executor `e`'s two plans."""
    return {"train": check_plan(e, e.plan, True), "eval": check_plan(e, e.eval_plan, False)}


def check_stats_plan(e) -> List[str]:
    """Errors of executor `e`'s `case_stats` op (`stats_plan`): it reads the probabilities
    the forward / evaluation plan left behind and the loaded target."""
    if e.stats_plan is None:
        return [e._case_stats_err]
    return check_plan(e, e.stats_plan, False, extra_inputs=("prob",))


def check_tta_plan(e) -> List[str]:
    """Errors of executor `e`'s test-time augmentation ops (`tta_plan`, built on first use or
    with --eval_tta): a tta_acc that writes the accumulator, one that adds to it and the
    finish.  They read the probabilities the evaluation plan left behind and the loaded
    target; the accumulator must be the size of `prob` and the partial buffer hold one row
    per block of the finish."""
    if e.tta_plan is None:
        return ["evaluate_tta is not planned (ExecutorBase.plan_tta)"]
    errs = check_plan(e, e.tta_plan, False, extra_inputs=("prob",))
    if e.tta_acc_buf.numel() != e.prob.numel() or e.tta_acc_buf.dtype != torch.float32:
        errs.append("evaluate_tta: tta_acc_buf holds %d floats, prob %d" % (e.tta_acc_buf.numel(), e.prob.numel()))
    need = tta_finish_blocks(e.prob.numel()) * 4
    if e.tta_partial.numel() < need:
        errs.append("evaluate_tta: tta_partial holds %d floats, %d needed" % (e.tta_partial.numel(), need))
    return errs


def check_sliding_plan(e) -> List[str]:
    """Errors of executor `e`'s sliding-window ops (`sw_plan`, built by `e.plan_sliding()` on first
    use): per batch of its probe geometry an sw_extract into the staging batch and an sw_blend
    of the probabilities the evaluation plan leaves behind, then the sw_finish.  The probe
    images, the weight maps and the summed weights are inputs; the accumulator is zeroed
    before the first batch.  The staging batch must hold one batch of fp32 tiles and the
    accumulator every image of the probe."""
    if e.sw_plan is None:
        return ["predict_sliding is not planned (ExecutorBase.plan_sliding)"]
    errs = check_plan(e, e.sw_plan, False, extra_inputs=("prob", "sw_src", "sw_w", "sw_wsum", "sw_acc"))
    d, h, w = e.sdims(1)
    need = e.B * d * h * w * e.spec.in_channels
    if e.sw_x.numel() != need or e.sw_x.dtype != torch.float32:
        errs.append("predict_sliding: sw_x holds %d floats, a batch of tiles %d" % (e.sw_x.numel(), need))
    return errs


def check_surface_plan(e) -> List[str]:
    """Errors of executor `e`'s `case_surface` op (`surface_plan`, built on first use or
    with --eval_hd95): like `case_stats` it reads the probabilities the forward /
    evaluation plan left behind and the loaded target.  The plan holds the op of the first
    group of samples; the output must hold every group's rows and the scratch one group."""
    if e.surface_plan is None:
        return [e._case_surface_err or "case_surface is not planned (ExecutorBase.plan_case_surface)"]
    errs = check_plan(e, e.surface_plan, False, extra_inputs=("prob",))
    K, (d, h, w) = e.K, e.sdims(1)
    if e.case_surface_buf.numel() < e.B * K * 4:
        errs.append("case_surface: case_surface_buf holds %d ints, B K 4 = %d needed"
                    % (e.case_surface_buf.numel(), e.B * K * 4))
    need = surf_dist_scratch(e._case_surface_group, d, h, w, K)
    have = e.case_surface_scratch.numel() * e.case_surface_scratch.element_size()
    if have < need:
        errs.append("case_surface: case_surface_scratch holds %d bytes, a group of %d samples needs %d"
                    % (have, e._case_surface_group, need))
    return errs


def check_components_plan(e) -> List[str]:
    """Errors of executor `e`'s `components` op (`components_plan`, built on first use or with
    --eval_components): it reads the probabilities the forward / evaluation plan left behind
    and writes `prob_pp`, `components_info` and the scratch.  The plan holds the op of the
    first group of samples; `prob_pp` must be the size of `prob`, the info hold every group's
    rows and the scratch one group."""
    if e.components_plan is None:
        return [e._components_err or "components is not planned (ExecutorBase.plan_components)"]
    errs = check_plan(e, e.components_plan, False, extra_inputs=("prob",))
    K, (d, h, w) = e.K, e.sdims(1)
    if e.prob_pp.numel() != e.prob.numel() or e.prob_pp.dtype != torch.float32:
        errs.append("components: prob_pp holds %d floats, prob %d" % (e.prob_pp.numel(), e.prob.numel()))
    if e.components_info.numel() < e.B * K * 4:
        errs.append("components: components_info holds %d ints, B K 4 = %d needed"
                    % (e.components_info.numel(), e.B * K * 4))
    need = components_scratch(e._components_group, d, h, w, K)
    have = e.components_scratch.numel() * e.components_scratch.element_size()
    if have < need:
        errs.append("components: components_scratch holds %d bytes, a group of %d samples needs %d"
                    % (have, e._components_group, need))
    return errs

"""What the 16-bit executor (`native_engine.NativeUNet`) and the fp32 one
(`f32_engine.NativeUNetF32`) share: loading a batch from the HBM-resident dataset and the
evaluation ops issued outside the step's plans (`case_stats`, `case_surface`, `components`,
`evaluate_tta`, `predict_sliding`), with the helpers of the same ops at the size of whole images.

A subclass plans and runs the training step.  Before it calls `_init_eval_ops` its `__init__`
sets `C`, `B`, `img`, `dims`, `device`, `spec`, `dtype`, `_dry`, `K` (classes of the head),
`dt_id` (the 16-bit type of its kernels; 0 for fp32), `cpad` (channels of the input buffer),
`bufs["x"]`, `target`, `prob`, `sums` and `eval_plan`; it provides `load_batch` and
`_load_plain` and names its build of the ops in `OP_PREFIX`.
"""

from contextlib import nullcontext as _nullctx
from typing import Optional, Tuple

import torch

from .. import native
from .plan_check import GATHER_OPS, RecordingPlan


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


# ops with one build for both executors (fp32 operands whatever the storage type): issued by
# their bare name; every other op of this module has an "f32_" twin for the fp32 executor
UNPREFIXED_OPS = frozenset(("tta_acc", "sw_extract", "sw_blend", "sw_finish", "components", "labelmap"))


def op_kind(name: str, prefix: str) -> str:
    """The kind (bindings.cpp) of op `name` in the build `prefix` ("" 16-bit, "f32_" fp32)."""
    return name if name in UNPREFIXED_OPS else prefix + name


def has_mat(aug) -> bool:
    """Whether the augmentation parameters `aug` end in warp matrices: (code, affine, mat)."""
    return aug is not None and len(aug) > 2 and aug[2] is not None


def has_field(aug) -> bool:
    """Whether the augmentation parameters `aug` end in an elastic field: (code, affine, mat or
    None, field)."""
    return aug is not None and len(aug) > 3 and aug[3] is not None


# cap of an executor's surf_dist scratch: the field is 8 bytes per (voxel, class) of a sample
# group, 384 MiB for K = 3 at b1024 128x128.  256 MiB keeps the 3D b8 128^3 K = 1 batch
# (128 MiB) and the 2D b1024 K = 1 batch (128 MiB) in one group and splits only the
# multi-class b1024 batches, into 2 groups of 512 samples that still fill the GPU.
SURF_SCRATCH_CAP = 256 << 20

# cap of an executor's components scratch: 8 bytes per (voxel, class) of a sample group (the
# int32 label and size planes), as surf_dist's fields: the same 256 MiB, the same groups
COMP_SCRATCH_CAP = SURF_SCRATCH_CAP


def surf_dist_group(N: int, sample_bytes: int, scratch_bytes: int) -> int:
    """Samples per surf_dist launch when the scratch holds `scratch_bytes` and one sample
    needs `sample_bytes`: the fewest groups that fit, of equal size but for the last."""
    fit = min(N, scratch_bytes // sample_bytes)
    if fit < 1:
        raise ValueError("surf_dist: the scratch (%d bytes) does not hold one sample (%d bytes)"
                         % (scratch_bytes, sample_bytes))
    groups = -(-N // fit)
    return -(-N // groups)


def launch_surf_dist(C, kind: str, ptrs, ints, threshold: float, scratch_bytes: int, target_bytes: int,
                     stream=0, dt_id: int = 0) -> int:
    """Issue `surf_dist` / `f32_surf_dist` (bindings.cpp) over N samples as immediate ops on
    groups of consecutive samples that fit the scratch.  ptrs = [prob, target, surf, scratch],
    ints = [N, D, H, W, K]; `target_bytes`: the target's element size.  prob, target and surf
    are sample-major, so a group is a pointer offset.  Returns the number of launches."""
    N, D, H, W, K = ints
    S = D * H * W
    g = surf_dist_group(N, C.surf_dist_scratch(1, D, H, W, K), scratch_bytes)
    prob, tgt, surf, scratch = ptrs
    n0 = launches = 0
    while n0 < N:
        n = min(g, N - n0)
        C.generic(kind, [prob + n0 * S * K * 4, tgt + n0 * S * K * target_bytes, surf + n0 * K * 16, scratch],
                  [n, D, H, W, K], [float(threshold)], stream, dt_id)
        n0 += n
        launches += 1
    return launches


def components_group(C, N: int, D: int, H: int, W: int, K: int, cap: int = COMP_SCRATCH_CAP) -> int:
    """Samples per `components` launch under the byte cap `cap` (at least one sample): the
    fewest groups that fit, of equal size but for the last.  ValueError with the op's reason
    where it refuses the shape."""
    C.components_scratch(1, D, H, W, K)                   # (the op's refusal of the shape, if any)
    lo, hi = 1, N                                         # the most samples whose scratch fits the cap
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if C.components_scratch(mid, D, H, W, K) <= cap:
            lo = mid
        else:
            hi = mid - 1
    groups = -(-N // lo)
    return -(-N // groups)


def launch_components(C, ptrs, ints, threshold: float, keep_largest: bool, min_size: int, group: int,
                      stream=0) -> int:
    """Issue `components` (bindings.cpp) over N samples as immediate ops on groups of `group`
    consecutive samples.  ptrs = [prob, out, info, scratch], ints = [N, D, H, W, K]; prob, out
    and info are sample-major, so a group is a pointer offset; the scratch holds
    components_scratch(group, ...) bytes.  Returns the number of launches (6 kernels each)."""
    N, D, H, W, K = ints
    S = D * H * W
    prob, out, info, scratch = ptrs
    n0 = launches = 0
    while n0 < N:
        n = min(group, N - n0)
        C.generic("components", [prob + n0 * S * K * 4, out + n0 * S * K * 4, info + n0 * K * 16, scratch],
                  [n, D, H, W, K, int(bool(keep_largest)), int(min_size)], [float(threshold)], stream, 0)
        n0 += n
        launches += 1
    return launches


def sliding_stats(C, prob: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, stream=None) -> torch.Tensor:
    """[N][K][6] = {I, St, Sp, TP, FP, FN} per (image, class) of full-size probabilities
    prob [N, (D,) H, W, K] (`predict_sliding`'s result) against the fp32 target y of the same
    shape: the fp32 `seg_stats` op at the images' own size, or `case_stats_torch` on the
    device (float64) where the op refuses the shape (S % 8, S >= 2^24, N S K >= 2^31)."""
    from ..ops import seg_metrics
    prob, y = prob.contiguous(), y.to(prob.device, torch.float32).contiguous()
    N, K = prob.shape[0], prob.shape[-1]
    S = prob[0].numel() // K
    try:
        chunks = C.seg_stats_chunks(N, S, K)
    except ValueError:
        return seg_metrics.case_stats_torch(prob, y, threshold)
    out = torch.zeros(N, K, 6, dtype=torch.float32, device=prob.device)
    part = torch.zeros(max(1, N * chunks * 6 * K), dtype=torch.float32, device=prob.device)
    C.generic(op_kind("seg_stats", "f32_"), [_ptr(prob), _ptr(y), _ptr(out), _ptr(part)], [N, S, K],
              [float(threshold)], native.stream_handle(stream), 0)
    return out


def sliding_surface(C, prob: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, stream=None) -> torch.Tensor:
    """int32 [N][K][4] = {mp, mt, q_lo, q_hi} per (image, class) of full-size probabilities
    against the fp32 target y: the fp32 `surf_dist` op at the images' own size in groups that fit
    SURF_SCRATCH_CAP, or `case_surface_torch` on the device where the op refuses the shape."""
    from ..ops import seg_metrics
    prob, y = prob.contiguous(), y.to(prob.device, torch.float32).contiguous()
    N, K = prob.shape[0], prob.shape[-1]
    d, h, w = tuple(prob.shape[1:4]) if prob.dim() == 5 else (1,) + tuple(prob.shape[1:3])
    try:
        one = C.surf_dist_scratch(1, d, h, w, K)
        C.surf_dist_scratch(N, d, h, w, K)
        group = surf_dist_group(N, one, max(one, min(one * N, SURF_SCRATCH_CAP)))
    except ValueError:
        return seg_metrics.case_surface_torch(prob, y, threshold).to(torch.int32)
    out = torch.zeros(N, K, 4, dtype=torch.int32, device=prob.device)
    scratch = torch.empty(one * group // 4, dtype=torch.int32, device=prob.device)
    launch_surf_dist(C, op_kind("surf_dist", "f32_"), [_ptr(prob), _ptr(y), _ptr(out), _ptr(scratch)],
                     [N, d, h, w, K], threshold, scratch.numel() * 4, 4, native.stream_handle(stream), 0)
    return out


def sliding_components(C, prob: torch.Tensor, threshold: float = 0.5, keep_largest: bool = True, min_size: int = 0,
                       stream=None, cap: int = COMP_SCRATCH_CAP):
    """(out fp32 like prob, info int32 [N][K][4]) of full-size probabilities prob [N, (D,) H, W, K]
    (`predict_sliding`'s result): the `components` op at the images' own size in groups
    that fit `cap`, or `components_torch` on the device where the op refuses the shape."""
    from ..ops import components as cc
    prob = prob.contiguous()
    N, K = prob.shape[0], prob.shape[-1]
    d, h, w = tuple(prob.shape[1:4]) if prob.dim() == 5 else (1,) + tuple(prob.shape[1:3])
    try:
        if C.components_check(N, d, h, w, K, int(min_size)) is not None:
            raise ValueError
        group = components_group(C, N, d, h, w, K, cap)
    except ValueError:
        out, info = cc.components_torch(prob, threshold, keep_largest, min_size)
        return out, info
    out = torch.empty_like(prob)
    info = torch.zeros(N, K, 4, dtype=torch.int32, device=prob.device)
    scratch = torch.empty(C.components_scratch(group, d, h, w, K) // 4, dtype=torch.int32, device=prob.device)
    launch_components(C, [_ptr(prob), _ptr(out), _ptr(info), _ptr(scratch)], [N, d, h, w, K], threshold,
                      keep_largest, min_size, group, native.stream_handle(stream))
    return out, info


def sliding_labels(C, prob: torch.Tensor, threshold: float = 0.5, rule: str = "nested", values=(1,),
                   out_shape=None, offset=(0, 0, 0), stream=None):
    """(labels uint8 [N, (Do,) Ho, Wo], counts int32 [N][K + 1]) on the device of full-size
    probabilities prob [N, (D,) H, W, K] (`predict_sliding`'s result, filtered or not), pasted at
    `offset` into `out_shape` (`ops.labelmap`): the `labelmap` op, or `labelmap_torch` on the
    device where the op refuses the launch."""
    from ..ops import labelmap as lm
    prob = prob.contiguous()
    N, (d, h, w), K, dst, off = lm.geometry(prob, out_shape, offset)
    values = lm.check_values(values, K)
    rule_id = lm.RULES.index(rule) if rule in lm.RULES else -1
    ints = [N, d, h, w, K] + list(dst) + list(off) + [rule_id, lm.pack_values(values)]
    if prob.dtype != torch.float32 or C.labelmap_check(*ints, float(threshold)) is not None:
        out, counts = lm.labelmap_torch(prob, threshold, rule, values, dst, off)
        return out, counts.to(torch.int32)
    out = torch.empty((N,) + dst, dtype=torch.uint8, device=prob.device)
    counts5 = torch.empty(N, 5, dtype=torch.int32, device=prob.device)
    C.generic("labelmap", [_ptr(prob), _ptr(out), _ptr(counts5)], ints, [float(threshold)],
              native.stream_handle(stream), 0)
    return (out if prob.dim() == 5 else out[:, 0]), counts5[:, :K + 1]


class ExecutorBase:
    """Shapes, the indexed load and the evaluation ops of an executor (see the module's text)."""

    OP_PREFIX = ""                  # "f32_": the fp32 build of the ops (op_kind)

    def _op(self, name: str) -> str:
        return op_kind(name, self.OP_PREFIX)

    def _live(self):
        """(the fp32 executor refuses to run the plans of a dry run)"""

    def _init_eval_ops(self, eval_hd95: bool, eval_tta: bool, eval_components: bool):
        """Plan `case_stats`; plan the ops that need buffers of their own only where the flag
        asks for them (otherwise on first use: the default trainer does not grow)."""
        self._iota = None
        self.plan_case_stats()
        self.surface_plan = self.case_surface_buf = self.case_surface_scratch = self._case_surface_err = None
        if eval_hd95:            # (otherwise on the first case_surface call)
            self.plan_case_surface()
        self.tta_plan = self.tta_acc_buf = self.tta_partial = None
        if eval_tta:             # (otherwise on the first evaluate_tta call)
            self.plan_tta()
        self.sw_plan = None      # (sliding-window inference: on the first predict_sliding call, or plan_sliding)
        self.components_plan = self.prob_pp = self.components_info = self.components_scratch = None
        self._components_err = None
        if eval_components:      # (otherwise on the first components call)
            self.plan_components()

    # ------------------------------------------------------------------ shapes
    def sdims(self, level: int) -> Tuple[int, int, int]:
        s = self.img >> (level - 1)
        return (s, s, s) if self.dims == 3 else (1, s, s)

    def npix(self, level: int) -> int:
        d, h, w = self.sdims(level)
        return self.B * d * h * w

    def probs(self) -> torch.Tensor:
        d, h, w = self.sdims(1)
        shape = (self.B, h, w, self.K) if self.dims == 2 else (self.B, d, h, w, self.K)
        return self.prob.view(shape)

    def probs_pp(self) -> torch.Tensor:
        """`prob_pp` in the shape of `probs()` (after a `components` call)."""
        return self.prob_pp.view(self.probs().shape)

    # ------------------------------------------------------------------ loading a batch
    def _batch_iota(self) -> torch.Tensor:
        """0 .. B-1 on the device: the index of a batch that is its own dataset."""
        if self._iota is None:
            self._iota = torch.arange(self.B, device=self.device, dtype=torch.int64)
        return self._iota

    def _check_indexed(self, x_all, y_all, idx):
        P = x_all[0].numel() // self.spec.in_channels
        assert idx.dtype == torch.int64 and idx.numel() == self.B and x_all.dtype == torch.float32
        assert y_all[0].numel() == P * self.K and x_all.is_contiguous() and y_all.is_contiguous()

    def _load_plain(self, x_all, y_all, idx, stream):
        """`load_indexed` without `aug` and `crop`: the subclass's own."""
        raise NotImplementedError

    def load_indexed(self, x_all: torch.Tensor, y_all: torch.Tensor, idx: torch.Tensor, stream=None, aug=None,
                     crop=None, elastic_cell: int = 32):
        """Batch = samples `idx` (device int64) of the HBM-resident dataset, gathered
        and cast straight into the (padded) input and the target (one launch).  `aug`:
        optional (code int32 [B], affine float32 [B][Cin][2] or None) on the device
        (data/augment.py): the same launch flips / rotates each sample and applies its
        per-channel affine (kernels/gather.h).  `crop`: optional (origin int32 [B][3] on
        the device, patch dims): the stored samples are larger than the model's input and the
        launch reads each sample's patch at its origin, then transforms it (the same kernels).
        An `aug` of three items (code or None, affine or None, mat int32 [B][4]) resamples the
        patch -- the whole sample without `crop` -- through each sample's matrix in the same
        launch (kernels/gather_resample.h).  An `aug` of four items (code or None, affine or None, mat or
        None, field int32 [B][N][N][2]) adds the elastic displacement of each sample's field to
        the warp's source coordinates (the same kernels): `elastic_cell` is the side S of a
        lattice cell in patch pixels and N = ((H - 1) >> log2 S) + 3.  A `mat` int32 [B][9] (3D
        executors) resamples trilinearly through 3 x 3 matrices over (d, h, w), with or without a field."""
        if aug is None and crop is None:
            return self._load_plain(x_all, y_all, idx, stream)
        self._check_indexed(x_all, y_all, idx)
        assert y_all.dtype == torch.float32
        name, ptrs, ints = self._gather_args(x_all, y_all, idx, aug, crop, elastic_cell)
        self.C.generic(self._op(name), ptrs, ints, [], native.stream_handle(stream), self.dt_id)

    def _gather_args(self, x_all, y_all, idx, aug, crop, elastic_cell: int = 32):
        """(op name, ptrs, ints) of the gather_batch_aug / _crop / _warp / _elastic / _warp3 launch (bindings.cpp)
        that loads the batch from the resident dataset [N, (Ds,) Hs, Ws, Cin]: `aug` = (code or
        None, affine or None[, mat int32 [B][4] or None]) or None, `crop` = (origin int32 [B][3],
        patch dims (D, H, W)) or None.  With `mat` it is the warp, whose patch without `crop` is
        the executor's input at origin 0, which the stored sample must hold; else with `crop`
        the crop; else the augmenting gather of whole samples, which needs its codes.  An `aug` of
        four items ends in the elastic field (int32 [B][N][N][2], cells of `elastic_cell` patch
        pixels) and selects the elastic op, whose `mat` may be None.  A `mat` int32 [B][9] (the
        3 x 3 matrices over (d, h, w)) selects gather_batch_warp3, with or without a field."""
        code, affine = aug[:2] if aug is not None else (None, None)
        mat = aug[2] if has_mat(aug) else None
        field = aug[3] if has_field(aug) else None
        if aug is not None and len(aug) > 3 and field is None:
            raise ValueError("an augmentation of four items ends in the elastic field")
        mat3 = mat is not None and mat.dim() == 2 and mat.shape[1] == 9
        name = "gather_batch_warp3" if mat3 else "gather_batch_elastic" if field is not None \
            else "gather_batch_warp" if mat is not None else "gather_batch_crop" if crop is not None \
            else "gather_batch_aug"
        B, cin, dev = self.B, self.spec.in_channels, x_all.device
        stored = (x_all.shape[1] if x_all.dim() == 5 else 1, x_all.shape[-3], x_all.shape[-2])
        origin, patch = crop if crop is not None else (None, self.sdims(1))
        patch = tuple(int(v) for v in patch)
        if name == "gather_batch_aug":
            assert stored == tuple(self.sdims(1))
        elif patch != tuple(self.sdims(1)):
            raise ValueError("crop patch %r: the executor's input is %r" % (patch, tuple(self.sdims(1))))
        if mat is not None or field is not None:
            if any(t > s for t, s in zip(patch, stored)):
                raise ValueError("the executor's input %r exceeds the stored sample %r" % (patch, stored))
        if field is not None:
            from ..data.augment import elastic_log2, elastic_nodes
            slog = elastic_log2(elastic_cell)
            N = elastic_nodes(patch[1], elastic_cell)
            if field.dtype != torch.int32 or tuple(field.shape) != (B, N, N, 2) or field.device != dev \
                    or not field.is_contiguous():
                raise ValueError("elastic field: a contiguous int32 [%d][%d][%d][2] tensor on %s (cell %d)"
                                 % (B, N, N, dev, elastic_cell))
        if mat is not None:
            # (a 2D executor takes the in-plane matrices alone, and its message says so)
            shapes = ((B, 4), (B, 9)) if self.dims == 3 else ((B, 4),)
            if mat.dtype != torch.int32 or tuple(mat.shape) not in shapes or mat.device != dev \
                    or not mat.is_contiguous():
                raise ValueError("warp matrices: a contiguous int32 [%d][4] %son %s" % (
                    B, "tensor " if self.dims != 3 else "(in-plane) or [%d][9] (over d, h, w) tensor " % B, dev))
        if (origin is not None or name == "gather_batch_crop") and (
                origin.dtype != torch.int32 or tuple(origin.shape) != (B, 3) or origin.device != dev
                or not origin.is_contiguous()):
            raise ValueError("crop origins: a contiguous int32 [%d][3] tensor on %s" % (B, dev))
        if (code is not None or name == "gather_batch_aug") and (
                code.dtype != torch.int32 or code.numel() != B or code.device != dev or not code.is_contiguous()):
            raise ValueError("augmentation codes: a contiguous int32 [%d] tensor on %s" % (B, dev))
        if affine is not None and (affine.dtype != torch.float32 or tuple(affine.shape) != (B, cin, 2)
                                   or affine.device != dev or not affine.is_contiguous()):
            raise ValueError("augmentation affine: a contiguous float32 [%d][%d][2] tensor on %s" % (B, cin, dev))
        row = GATHER_OPS[name]
        own = {"origin": origin, "code": code, "mat": mat, "affine": affine, "field": field}
        ptrs = [x_all, y_all, idx] + [own[k] for k in row.slots] + [self.bufs["x"], self.target]
        ints = [B] + (list(stored) if row.patch == 4 else []) + list(patch) + [cin, self.cpad, self.K] + (
            [slog if field is not None else 0] if "field" in row.slots else [])
        return name, [0 if t is None else _ptr(t) for t in ptrs], ints

    # ------------------------------------------------------------------ evaluation
    def evaluate_batch(self, stream=None):
        """Inference forward (eval plan) of the loaded batch; sums -> self.sums."""
        self._live()
        self.eval_plan.set_seed(0)
        self.eval_plan.run(0, self.eval_plan.size(), native.stream_handle(stream))

    def _refuse_dry(self, what: str):
        if self._dry:
            raise RuntimeError("executor built with dry_run=True: %s is validated, not launched" % what)

    def _post_args(self, args):
        """The argument set (ptrs, ints) of `case_stats` / `case_surface` with `prob_pp` for `prob`."""
        if self.prob_pp is None:
            raise RuntimeError("no filtered probabilities: call components() before scoring prob_pp")
        ptrs, ints = args
        return [_ptr(self.prob_pp)] + list(ptrs[1:]), ints

    def plan_case_stats(self) -> None:
        """Buffers and the validation plan of `case_stats` (kernels/seg_stats.h).

        The op is not part of `plan` / `eval_plan`: `stats_plan` holds it alone (threshold 0.5)
        so the static plan validation covers its layout and extents on a dry-run executor;
        `case_stats` issues it as an immediate op with the caller's threshold."""
        K = self.K
        S = self.npix(1) // self.B
        self.case_stats_buf = self.case_stats_partial = self.stats_plan = None
        try:
            chunks = self.C.seg_stats_chunks(self.B, S, K)
        except ValueError as err:               # (e.g. 2^24 voxels per sample: fp32 counts not exact)
            self._case_stats_err = str(err)
            return
        self._case_stats_err = None
        self.case_stats_buf = torch.zeros(self.B, K, 6, dtype=torch.float32, device=self.device)
        self.case_stats_partial = torch.zeros(max(1, self.B * chunks * 6 * K), dtype=torch.float32,
                                              device=self.device)
        self._case_stats_args = ([_ptr(self.prob), _ptr(self.target), _ptr(self.case_stats_buf),
                                  _ptr(self.case_stats_partial)], [self.B, S, K])
        self.stats_plan = RecordingPlan(self.C.Plan(self.dt_id))
        self.stats_plan.add_generic(self._op("seg_stats"), self._case_stats_args[0], self._case_stats_args[1], [0.5],
                                    "case_stats")

    def case_stats(self, threshold: float = 0.5, stream=None, post: bool = False) -> torch.Tensor:
        """[B][K][6] = {I, St, Sp, TP, FP, FN} per (sample, class) of the probabilities and
        target the last forward / evaluate_batch left behind (one launch, seg_stats.h; the
        returned tensor is the executor's buffer, overwritten by the next call).  `post`: of the
        filtered probabilities `prob_pp` the last `components` call left behind."""
        if self._case_stats_err is not None:
            raise ValueError(self._case_stats_err)
        self._refuse_dry("case_stats")
        ptrs, ints = self._post_args(self._case_stats_args) if post else self._case_stats_args
        self.C.generic(self._op("seg_stats"), ptrs, ints, [float(threshold)], native.stream_handle(stream),
                       self.dt_id)
        return self.case_stats_buf

    def plan_case_surface(self) -> None:
        """Buffers and the validation plan of `case_surface` (kernels/surf_dist.h): the int32
        [B][K][4] output and the field scratch, min(one batch, SURF_SCRATCH_CAP).

        Like `case_stats` the op is in neither `plan` nor `eval_plan`: `surface_plan` holds the
        op of the first sample group alone (threshold 0.5) for the static plan validation."""
        K = self.K
        d, h, w = self.sdims(1)
        try:
            need = self.C.surf_dist_scratch(self.B, d, h, w, K)
            group = surf_dist_group(self.B, need // self.B, min(need, SURF_SCRATCH_CAP))
        except ValueError as err:
            self._case_surface_err = str(err)
            return
        self._case_surface_group = group
        self.case_surface_buf = torch.zeros(self.B, K, 4, dtype=torch.int32, device=self.device)
        self.case_surface_scratch = torch.empty(need // self.B * group // 4, dtype=torch.int32, device=self.device)
        self._case_surface_args = ([_ptr(self.prob), _ptr(self.target), _ptr(self.case_surface_buf),
                                    _ptr(self.case_surface_scratch)], [self.B, d, h, w, K])
        self.surface_plan = RecordingPlan(self.C.Plan(self.dt_id))
        self.surface_plan.add_generic(self._op("surf_dist"), self._case_surface_args[0], [group, d, h, w, K], [0.5],
                                      "case_surface")

    def case_surface(self, threshold: float = 0.5, stream=None, post: bool = False) -> torch.Tensor:
        """int32 [B][K][4] = {mp, mt, q_lo, q_hi} per (sample, class): the surface sizes of
        {prob >= threshold} and {target >= 0.5} and the two squared surface distances that
        bracket the 95th percentile (`ops.seg_metrics.hd95_from_surface`), of the
        probabilities and target the last forward / evaluate_batch left behind (surf_dist.h).
        The returned tensor is the executor's buffer, overwritten by the next call.  `post`: of
        the filtered probabilities `prob_pp` the last `components` call left behind."""
        self._refuse_dry("case_surface")
        if self.surface_plan is None and self._case_surface_err is None:
            self.plan_case_surface()
        if self._case_surface_err is not None:
            raise ValueError(self._case_surface_err)
        ptrs, ints = self._post_args(self._case_surface_args) if post else self._case_surface_args
        launch_surf_dist(self.C, self._op("surf_dist"), ptrs, ints, threshold, self.case_surface_scratch.numel() * 4,
                         self.target.element_size(), native.stream_handle(stream), self.dt_id)
        return self.case_surface_buf

    def plan_components(self) -> None:
        """Buffers and the validation plan of `components` (kernels/components.h): `prob_pp`
        (the size of `prob`), the int32 [B][K][4] `components_info` and the scratch of one
        sample group under COMP_SCRATCH_CAP.  `case_stats` / `case_surface` score `prob_pp` in
        place of `prob` with `post`.

        Like `case_stats` the op is in neither `plan` nor `eval_plan`: `components_plan` holds the
        op of the first sample group alone (threshold 0.5, keep the largest) for the static plan
        validation."""
        K = self.K
        d, h, w = self.sdims(1)
        try:
            group = components_group(self.C, self.B, d, h, w, K)
            need = self.C.components_scratch(group, d, h, w, K)
        except ValueError as err:
            self._components_err = str(err)
            return
        self._components_group = group
        self.prob_pp = torch.zeros_like(self.prob)
        self.components_info = torch.zeros(self.B, K, 4, dtype=torch.int32, device=self.device)
        self.components_scratch = torch.empty(need // 4, dtype=torch.int32, device=self.device)
        self._components_args = ([_ptr(self.prob), _ptr(self.prob_pp), _ptr(self.components_info),
                                  _ptr(self.components_scratch)], [self.B, d, h, w, K])
        self.components_plan = RecordingPlan(self.C.Plan(self.dt_id))
        self.components_plan.add_generic(self._op("components"), self._components_args[0],
                                         [group, d, h, w, K, 1, 0], [0.5], "components")

    def components(self, threshold: float = 0.5, keep_largest: bool = True, min_size: int = 0,
                   stream=None) -> torch.Tensor:
        """Connected-component filter (kernels/components.h, `ops.components` is the
        definition) of the probabilities the last forward / evaluate_batch left behind:
        `prob_pp` (see `probs_pp`) holds the filtered map and the returned int32 [B][K][4] =
        {components, kept components, largest size, kept voxels} is the executor's buffer."""
        self._refuse_dry("components")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError("components: threshold strictly inside (0, 1)")
        if int(min_size) < 0:
            raise ValueError("components: min_size >= 0")
        if self.components_plan is None and self._components_err is None:
            self.plan_components()
        if self._components_err is not None:
            raise ValueError(self._components_err)
        ptrs, ints = self._components_args
        launch_components(self.C, ptrs, ints, threshold, keep_largest, min_size, self._components_group,
                          native.stream_handle(stream))
        return self.components_info

    def plan_tta(self) -> None:
        """Buffers and the validation plan of `evaluate_tta` (kernels/tta.h): the accumulator,
        the size of `prob`, and the finish's block partials.  Like `case_stats` the ops are in
        neither `plan` nor `eval_plan`: `tta_plan` holds one tta_acc that writes, one that adds
        and the finish (M = 4) for the static plan validation; the [M][B] code rows of a code
        set are made on its first use."""
        d, h, w = self.sdims(1)
        total = self.prob.numel()
        self.tta_acc_buf = torch.empty_like(self.prob)
        self.tta_partial = torch.zeros(self.C.tta_finish_blocks(total) * 4, dtype=torch.float32, device=self.device)
        self._tta_rows = {}
        self._tta_acc_args = ([_ptr(self.prob), _ptr(self.tta_acc_buf)], [self.B, d, h, w, self.K])
        self._tta_finish_args = ([_ptr(self.prob), _ptr(self.tta_acc_buf), _ptr(self.target), _ptr(self.tta_partial),
                                  _ptr(self.sums)], [total])
        self.tta_plan = RecordingPlan(self.C.Plan(self.dt_id))
        ptrs, ints = self._tta_acc_args
        # (code 1 = FW: the strip path; code 5 = T | FW: the tile path)
        self.tta_plan.add_generic(self._op("tta_acc"), ptrs, ints + [1, 0], [], "tta_acc:write")
        self.tta_plan.add_generic(self._op("tta_acc"), ptrs, ints + [5, 1], [], "tta_acc:add")
        self.tta_plan.add_generic(self._op("tta_finish"), self._tta_finish_args[0], self._tta_finish_args[1], [0.25],
                                  "tta_finish")

    def evaluate_tta(self, x: torch.Tensor, y: torch.Tensor, codes, stream=None) -> None:
        """Test-time augmentation of one batch x [B, (D,) H, W, Cin], y [B, (D,) H, W, K] over the
        transform codes `codes` (data/augment.py tta_codes: a power of two of them, the identity
        last).  Per non-identity code: the augmenting gather loads the transformed batch, the
        evaluation plan runs, tta_acc brings `prob` back by the inverse code into the accumulator
        (the first writes it, the others add).  The identity pass goes through the same gather,
        then tta_finish forms the mean in place.  Afterwards `prob` holds the mean, `target` the
        stored target and `sums` the sums of the mean (BCE from the probabilities), so
        `case_stats`, `case_surface` and `probs()` work unchanged."""
        from ..data.augment import inverse_code
        self._refuse_dry("evaluate_tta")
        codes = tuple(int(c) for c in codes)
        M = len(codes)
        if M < 2 or M & (M - 1) or codes[-1] != 0 or 0 in codes[:-1] or len(set(codes)) != M:
            raise ValueError("evaluate_tta: a power of two >= 2 of distinct codes with the identity last, got %r"
                             % (codes,))
        if x.shape[0] != self.B:
            raise ValueError("evaluate_tta takes the executor's batch of %d samples, got %d" % (self.B, x.shape[0]))
        if self.tta_plan is None:
            self.plan_tta()
        # (inputs that are not fp32 / contiguous / on the device are converted first)
        x = x.to(self.device, torch.float32).contiguous()
        y = y.to(self.device, torch.float32).contiguous()
        rows = self._tta_rows.get(codes)
        if rows is None:
            rows = self._tta_rows[codes] = \
                torch.tensor(codes, dtype=torch.int32).view(M, 1).repeat(1, self.B).to(self.device)
        iota = self._batch_iota()
        s, dt = native.stream_handle(stream), self.dt_id
        ptrs, ints = self._tta_acc_args
        for i, c in enumerate(codes):
            self.load_indexed(x, y, iota, stream, aug=(rows[i], None))
            self.evaluate_batch(stream)
            if c:
                self.C.generic(self._op("tta_acc"), ptrs, ints + [inverse_code(c), 1 if i else 0], [], s, dt)
        self.C.generic(self._op("tta_finish"), self._tta_finish_args[0], self._tta_finish_args[1], [1.0 / M], s, dt)

    def plan_sliding(self) -> None:
        """Buffers and the validation plan of `predict_sliding` (kernels/sliding.h, `ops.sliding`
        is the definition): the fp32 staging batch `sw_x` of B tiles of the model's size that
        `sw_extract` fills and the plain load consumes, the zero target that rides along, and
        the device weight maps `sw_w` [constant, gaussian].  Like `case_stats` the ops are in
        neither `plan` nor `eval_plan`: `sw_plan` holds the ops of a probe geometry -- one image
        a quarter tile wider than the tile at overlap 0.5, two tiles with the second clamped --
        for the static plan validation; the accumulator and summed weights of a real call are
        made per geometry by `predict_sliding`."""
        from ..ops import sliding
        B, K, cin = self.B, self.K, self.spec.in_channels
        T = self.sdims(1)
        sp = T if self.dims == 3 else T[1:]
        self.sw_x = torch.zeros((B,) + sp + (cin,), dtype=torch.float32, device=self.device)
        self.sw_y = torch.zeros((B,) + sp + (K,), dtype=torch.float32, device=self.device)
        self.sw_w = torch.stack([sliding.weight_map(T, b) for b in sliding.BLENDS]).to(self.device)
        self._sw_run = None
        dims = (T[0], T[1], T[2] + max(1, T[2] // 4))
        stride = sliding.strides(T, 0.5)
        self.sw_src = torch.zeros((1,) + dims + (cin,), dtype=torch.float32, device=self.device)
        self.sw_acc = torch.zeros((1,) + dims + (K,), dtype=torch.float32, device=self.device)
        self.sw_wsum = sliding.weight_sum(dims, T, stride, "gaussian").to(self.device)
        plan = self.sw_plan = RecordingPlan(self.C.Plan(self.dt_id))
        total = sliding.tiles_per_image(dims, T, stride)
        for t0 in range(0, total, B):
            tail = list(T) + list(stride) + [B, t0, min(B, total - t0)]
            plan.add_generic(self._op("sw_extract"), [_ptr(self.sw_src), _ptr(self.sw_x)],
                             [1] + list(dims) + [cin] + tail, [], "sw_extract:%d" % t0)
            plan.add_generic(self._op("sw_blend"), [_ptr(self.prob), _ptr(self.sw_w[1]), _ptr(self.sw_acc)],
                             [1] + list(dims) + [K] + tail, [], "sw_blend:%d" % t0)
        plan.add_generic(self._op("sw_finish"), [_ptr(self.sw_acc), _ptr(self.sw_wsum)], [1] + list(dims) + [K], [],
                         "sw_finish")

    def predict_sliding(self, x: torch.Tensor, overlap: float = 0.5, blend: str = "gaussian", tta_codes=(),
                        stream=None) -> torch.Tensor:
        """Sliding-window probabilities of the images x [N, (D,) H, W, Cin] of any spatial size
        (`ops.sliding`): zero the accumulator; per batch of B tiles `sw_extract` fills the staging
        batch, the evaluation forward runs on it (the plain load and plan, or `evaluate_tta` over
        `tta_codes`) and `sw_blend` adds the weighted probabilities; `sw_finish` divides by the
        summed weights.  Everything is issued in order on one stream, so every pixel's sum runs
        in ascending tile order, as the oracle's.  Returns fp32 [N, (D,) H, W, K] on the device:
        the executor's buffer, overwritten by the next call of the same geometry."""
        from ..ops import sliding
        self._refuse_dry("predict_sliding")
        sliding.check_blend(blend)
        T = self.sdims(1)
        stride = sliding.strides(T, overlap)
        B, K, cin = self.B, self.K, self.spec.in_channels
        if x.dim() != self.dims + 2 or x.shape[-1] != cin or x.shape[0] < 1:
            raise ValueError("predict_sliding: images [n, %sH, W, %d], got shape %r"
                             % ("D, " if self.dims == 3 else "", cin, tuple(x.shape)))
        if self.sw_plan is None:
            self.plan_sliding()
        x = x.to(self.device, torch.float32).contiguous()
        N = x.shape[0]
        dims = tuple(x.shape[1:4]) if self.dims == 3 else (1,) + tuple(x.shape[1:3])
        key = (N, dims, stride, blend)
        run = self._sw_run
        if run is None or run["key"] != key:
            self._sw_run = None                   # (the previous geometry's buffers go first)
            run = self._sw_run = dict(key=key,
                                      acc=torch.empty((N,) + dims + (K,), dtype=torch.float32, device=self.device),
                                      wsum=sliding.weight_sum(dims, T, stride, blend).to(self.device))
        acc, w = run["acc"], self.sw_w[sliding.BLENDS.index(blend)]
        total = N * sliding.tiles_per_image(dims, T, stride)
        s, dt = native.stream_handle(stream), self.dt_id
        with torch.cuda.stream(stream) if stream is not None else _nullctx():
            acc.zero_()
        head = [N] + list(dims)
        for t0 in range(0, total, B):
            tail = list(T) + list(stride) + [B, t0, min(B, total - t0)]
            self.C.generic(self._op("sw_extract"), [_ptr(x), _ptr(self.sw_x)], head + [cin] + tail, [], s, dt)
            if tta_codes:
                self.evaluate_tta(self.sw_x, self.sw_y, tta_codes, stream)
            else:
                self.load_batch(self.sw_x, self.sw_y, stream)
                self.evaluate_batch(stream)
            self.C.generic(self._op("sw_blend"), [_ptr(self.prob), _ptr(w), _ptr(acc)], head + [K] + tail, [], s, dt)
        self.C.generic(self._op("sw_finish"), [_ptr(acc), _ptr(run["wsum"])], head + [K], [], s, dt)
        return acc if self.dims == 3 else acc.view((N,) + dims[1:] + (K,))

"""Step backends: one forward + backward of the local micro-batch into the flat
gradient buffer.

* ``NativeBackend`` -- the MI355X path: the planned HIP executor
  (``runtime.native_engine.NativeUNet``).  Mandatory on GPU for the configs
  it supports; never silently replaced by ATen.
* ``TorchBackend`` -- ATen reference (CPU plumbing config, fp32 runs, and the
  numerical oracle for the kernels).

Both expose ``fwd_bwd(x, y, seed, on_segment)``, ``sums()`` (device tensor
{I, St, Sp, BCE_sum} of the last forward), ``eval_sums(x, y)`` and the per-(sample,
class) statistics of ``ops.seg_metrics``: ``last_eval_stats(threshold)`` of the batch the
last ``eval_sums`` scored (no second forward) and ``eval_stats(x, y, threshold)``; likewise
``last_eval_surface`` / ``eval_surface`` for the surface-distance integers of HD95.
With ``--eval_tta`` every one of these evaluation forwards (``predict`` too) is the mean of
the probabilities over the flipped / rotated inputs (``data.augment.tta_mean_torch`` on
ATen, the executors' ``evaluate_tta`` on the HIP path); training steps are untouched.
``predict_sliding(x, overlap, blend)`` scores images of any spatial size by sliding-window
inference (``ops.sliding``: the torch loop on ATen, the executors' ``predict_sliding`` with
the sw_extract / sw_blend / sw_finish kernels on the HIP path); ``sliding_stats`` /
``sliding_surface`` score its full-size result against a full-size target.
With ``--eval_components`` the per-case methods (``*_stats``, ``*_surface``) score the
connected-component-filtered map (``ops.components``: the torch definition on ATen, the
executors' ``components`` op on the HIP path), ``predict`` / ``predict_sliding`` return it and
``last_eval_components`` / ``eval_components`` give its ``info`` rows; with --eval_tta the
filter applies to the mean, with sliding windows to the blended full-size map.  ``eval_sums``
never sees the filter.
"""

from typing import Callable, Optional

import torch

from ..data.augment import tta_codes, tta_mean_torch
from ..models import reference
from ..config import parse_components
from ..ops import components as cc
from ..ops import losses, seg_metrics, sliding
from .params import FlatParams


class TorchBackend:
    name = "torch"

    def __init__(self, spec, flat: FlatParams, cfg, device, per_rank_batch: int, bounds=None):
        self.spec = spec
        self.flat = flat
        self.cfg = cfg
        self.device = torch.device(device)
        self.B = per_rank_batch               # (tiles per forward of predict_sliding)
        self.dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[cfg.dtype]
        if self.device.type == "cpu" and self.dtype == torch.float16:
            self.dtype = torch.float32
        self._sums = torch.zeros(4, device=self.device)
        self.state = {}
        if spec.norm == "batch":
            for l in spec.param_layers():
                if l.kind == "conv":
                    self.state[l.name + "/norm/moving_mean"] = torch.zeros(l.cout, device=self.device)
                    self.state[l.name + "/norm/moving_variance"] = torch.ones(l.cout, device=self.device)
        # allreduce buckets: on_segment(k) is called once per bucket after the backward
        # (the GradSync of the trainer is planned with the same bounds)
        self.bounds = list(bounds) if bounds else [flat.numel]
        # --eval_tta: the transform codes every evaluation forward is averaged over (() = off)
        self.tta = tta_codes(getattr(cfg, "eval_tta", ""), spec.dims)
        # --eval_components: the policy (keep_largest, min_size) of the per-case scores (None = off)
        self.components = _policy(cfg)
        self._pp = None                       # (probabilities, threshold, filtered map, info) last filtered

    def set_buckets(self, bounds):
        self.bounds = list(bounds)

    def _filter(self, p, threshold: float):
        """(p, None) with the filter off, else (filtered p, info) of `ops.components`; the last
        result is kept, so the stats, surface and info of one batch filter once, and a map
        that is itself the last result (``predict_sliding``'s) is not filtered again."""
        if self.components is None:
            return p, None
        c = self._pp
        if c is not None and c[1] == threshold and (c[0] is p or c[2] is p):
            return c[2], c[3]
        out, info = cc.components_torch(p, threshold, *self.components)
        self._pp = (p, threshold, out, info)
        return out, info

    def _forward_logits(self, params, x, train, seed, dropout):
        with torch.autocast(self.device.type, dtype=self.dtype, enabled=self.dtype != torch.float32):
            return reference.forward(self.spec, params, x.to(self.device), train=train, dropout=dropout,
                                     seed=seed, state=self.state, return_logits=True)

    def fwd_bwd(self, x, y, seed: int, on_segment: Optional[Callable[[int], None]] = None,
                grad_scale: float = 1.0):
        if hasattr(x, "x_all"):
            x, y = x.tensors()
        names = [e[0] for e in self.flat.entries]
        leaves = {n: self.flat.view(self.flat.master, n).detach().requires_grad_(True) for n in names}
        logits = self._forward_logits(leaves, x, True, seed, True).float()
        t = y.to(self.device).float()
        loss, p = losses.total_loss(t, logits, self.cfg.loss, self.cfg.bce_weight)
        grads = torch.autograd.grad(loss * grad_scale, [leaves[n] for n in names], allow_unused=True)
        for n, g in zip(names, grads):
            gv = self.flat.view(self.flat.grad, n)
            if g is None:
                gv.zero_()
            else:
                gv.copy_(g)
        with torch.no_grad():
            i, st, sp = losses.dice_sums(t, p)
            bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, t, reduction="sum")
            self._sums = torch.stack([i, st, sp, bce]).detach()
        self._last = (x, t, p.detach())
        if on_segment is not None:
            for k in range(len(self.bounds)):
                on_segment(k)

    def sums(self) -> torch.Tensor:
        return self._sums

    def summary_images(self, n: int) -> dict:
        """First n samples of the last training batch (channel 0; 3D: middle slice)."""
        x, t, p = self._last
        return _summary_arrays(x, t[..., :1], p[..., :1], n)     # (several output classes: class 0)

    @torch.no_grad()
    def eval_sums(self, x, y) -> torch.Tensor:
        t = y.to(self.device).float()
        if self.tta:
            # the mean probability has no logits: BCE from the probabilities (log clamped at -100)
            p = self._predict_raw(x)
            self._last_eval = (t, p)
            i, st, sp = losses.dice_sums(t, p)
            return torch.stack([i, st, sp, torch.nn.functional.binary_cross_entropy(p, t, reduction="sum")])
        logits = self._forward_logits(self.flat.params(), x, False, 0, self.cfg.eval_dropout).float()
        p = torch.sigmoid(logits)
        self._last_eval = (t, p)
        i, st, sp = losses.dice_sums(t, p)
        bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, t, reduction="sum")
        return torch.stack([i, st, sp, bce])

    @torch.no_grad()
    def last_eval_stats(self, threshold: float = 0.5) -> torch.Tensor:
        """[n][K][6] of the batch the last ``eval_sums`` scored."""
        t, p = self._last_eval
        return seg_metrics.case_stats_torch(self._filter(p, threshold)[0], t, threshold)

    @torch.no_grad()
    def eval_stats(self, x, y, threshold: float = 0.5) -> torch.Tensor:
        """[n][K][6] = {I, St, Sp, TP, FP, FN} per (sample, class) of the n samples given."""
        p = self._filter(self._predict_raw(x), threshold)[0]
        return seg_metrics.case_stats_torch(p, y.to(self.device).float(), threshold)

    @torch.no_grad()
    def last_eval_surface(self, threshold: float = 0.5) -> torch.Tensor:
        """[n][K][4] = {mp, mt, q_lo, q_hi} of the batch the last ``eval_sums`` scored."""
        t, p = self._last_eval
        return seg_metrics.case_surface_torch(self._filter(p, threshold)[0], t, threshold)

    @torch.no_grad()
    def eval_surface(self, x, y, threshold: float = 0.5) -> torch.Tensor:
        """[n][K][4] = {mp, mt, q_lo, q_hi} per (sample, class) of the n samples given."""
        p = self._filter(self._predict_raw(x), threshold)[0]
        return seg_metrics.case_surface_torch(p, y.to(self.device).float(), threshold)

    @torch.no_grad()
    def last_eval_components(self, threshold: float = 0.5) -> torch.Tensor:
        """int32 [n][K][4] = {components, kept components, largest size, kept voxels} of the
        batch the last ``eval_sums`` scored (--eval_components)."""
        _need_policy(self)
        return self._filter(self._last_eval[1], threshold)[1]

    @torch.no_grad()
    def eval_components(self, x, y=None, threshold: float = 0.5) -> torch.Tensor:
        """int32 [n][K][4] per (sample, class) of the n samples given (y is not used)."""
        _need_policy(self)
        return self._filter(self._predict_raw(x), threshold)[1]

    def _predict1(self, x) -> torch.Tensor:
        logits = self._forward_logits(self.flat.params(), x, False, 0, self.cfg.eval_dropout).float()
        return torch.sigmoid(logits)

    def _predict_raw(self, x) -> torch.Tensor:
        if self.tta:
            return tta_mean_torch(self._predict1, x.to(self.device), self.tta)
        return self._predict1(x)

    @torch.no_grad()
    def predict(self, x) -> torch.Tensor:
        """Probabilities of x; with --eval_tta their mean over the transforms (`tta_mean_torch`);
        with --eval_components filtered at --eval_threshold."""
        return self._filter(self._predict_raw(x), getattr(self.cfg, "eval_threshold", 0.5))[0]

    @torch.no_grad()
    def predict_sliding(self, x, overlap: float = 0.5, blend: str = "gaussian", post: bool = True) -> torch.Tensor:
        """Probabilities fp32 [n, (D,) H, W, K] of images of any spatial size: `predict` on
        overlapping tiles of the model's size, blended (`ops.sliding.sliding_predict_torch`).
        post=False: the blended map itself, before the --eval_components filter."""
        T = sliding.tile_shape(self.cfg.img_size, self.spec.dims)
        p = sliding.sliding_predict_torch(self._predict_raw, x.to(self.device), T, self.B, overlap, blend)
        return self._filter(p, getattr(self.cfg, "eval_threshold", 0.5))[0] if post else p

    @torch.no_grad()
    def sliding_filter(self, p, threshold: float = 0.5) -> torch.Tensor:
        """The --eval_components filter of full-size probabilities p (p itself with the flag
        off): what `predict_sliding` returns, from its post=False map."""
        return self._filter(p, threshold)[0]

    @torch.no_grad()
    def sliding_components(self, p, threshold: float = 0.5) -> torch.Tensor:
        """int32 [n][K][4] of full-size probabilities p (`predict_sliding`'s result)."""
        _need_policy(self)
        return self._filter(p, threshold)[1]

    @torch.no_grad()
    def sliding_stats(self, p, y, threshold: float = 0.5, post: bool = True) -> torch.Tensor:
        """[n][K][6] of full-size probabilities p (`predict_sliding`) against the target y.
        post=False: of p itself, the --eval_components filter not applied."""
        return seg_metrics.case_stats_torch(self._filter(p, threshold)[0] if post else p, y.to(p.device).float(),
                                            threshold)

    @torch.no_grad()
    def sliding_surface(self, p, y, threshold: float = 0.5, post: bool = True) -> torch.Tensor:
        """[n][K][4] of full-size probabilities p (`predict_sliding`) against the target y.
        post=False: of p itself, the --eval_components filter not applied."""
        return seg_metrics.case_surface_torch(self._filter(p, threshold)[0] if post else p, y.to(p.device).float(),
                                              threshold)

    @torch.no_grad()
    def filter_once(self, p, threshold: float = 0.5):
        """(filtered p, info or None) of the --eval_components filter, the kept last result neither
        used nor replaced (`Predictor.segment`: a case's map is filtered under another shape)."""
        if self.components is None:
            return p, None
        return cc.components_torch(p, threshold, *self.components)

    @torch.no_grad()
    def sliding_labels(self, p, threshold: float = 0.5, rule: str = "nested", values=(1,), out_shape=None,
                       offset=(0, 0, 0)):
        """(labels uint8, counts int32 [n][K + 1]) of full-size probabilities p (`ops.labelmap`)."""
        from ..ops import labelmap
        out, counts = labelmap.labelmap_torch(p, threshold, rule, values, out_shape, offset)
        return out, counts.to(torch.int32)

    def after_optimizer(self):
        pass


class NativeBackend:
    name = "native"

    def __init__(self, spec, flat: FlatParams, cfg, device, per_rank_batch: int, bounds=None):
        from .native_engine import NativeUNet
        from .f32_engine import NativeUNetF32
        self.cfg = cfg
        self.flat = flat
        self.spec = spec
        # --eval_tta: the transform codes every evaluation forward is averaged over (() = off)
        self.tta = tta_codes(getattr(cfg, "eval_tta", ""), spec.dims)
        # --eval_components: the policy (keep_largest, min_size) of the per-case scores (None = off)
        self.components = _policy(cfg)
        self._pp_thr = None                   # threshold at which prob_pp is the filter of the executor's prob
        self._sw_pp = None                    # (probabilities, threshold, filtered map, info) of a full-size map
        if cfg.dtype == "fp32":
            # the reference's precision (test_dist.py:196-202): fp32 storage, fp32 MFMA
            self.engine = NativeUNetF32(spec, flat, per_rank_batch, cfg.img_size, device, loss=cfg.loss,
                                        bce_weight=cfg.bce_weight, bucket_bounds=bounds,
                                        eval_dropout=cfg.eval_dropout, eval_hd95=getattr(cfg, "eval_hd95", False),
                                        eval_tta=bool(self.tta), eval_components=self.components is not None)
        else:
            self.engine = NativeUNet(spec, flat, per_rank_batch, cfg.img_size, device, loss=cfg.loss,
                                     bce_weight=cfg.bce_weight, bucket_bounds=bounds,
                                     eval_dropout=cfg.eval_dropout, dtype=cfg.dtype,
                                     eval_hd95=getattr(cfg, "eval_hd95", False), eval_tta=bool(self.tta),
                                     eval_components=self.components is not None)
        self.B = per_rank_batch
        if getattr(cfg, "hip_graph", False):
            self.engine.enable_graphs()
        self.state = self.engine.state        # BatchNorm running statistics (checkpointed)

    def set_buckets(self, bounds):
        self.engine.set_buckets(bounds)

    def fwd_bwd(self, x, y, seed: int, on_segment=None, grad_scale: float = 1.0):
        """x, y: batch tensors, or x = a data.loader.ResidentBatch (y unused)."""
        e = self.engine
        self._pp_thr = None
        e.set_loss_scale(grad_scale)
        if hasattr(x, "x_all"):
            if getattr(x, "aug", None) is not None and len(x.aug) > 3:      # --augment elastic: the field's cell
                e.load_indexed(x.x_all, x.y_all, x.idx, aug=x.aug, crop=getattr(x, "crop", None),
                               elastic_cell=x.elastic_cell)
            elif getattr(x, "crop", None) is not None:
                e.load_indexed(x.x_all, x.y_all, x.idx, aug=x.aug, crop=x.crop)
            elif getattr(x, "aug", None) is not None:
                e.load_indexed(x.x_all, x.y_all, x.idx, aug=x.aug)
            else:
                e.load_indexed(x.x_all, x.y_all, x.idx)
        else:
            e.load_batch(x, y)
        e.forward(seed)
        e.backward(on_segment)

    def sums(self) -> torch.Tensor:
        return self.engine.sums

    def summary_images(self, n: int) -> dict:
        """From the buffers the step already holds (no extra forward, Q8): the padded
        16-bit input, the target and the head's probabilities."""
        e = self.engine
        d, h, w = e.sdims(1)
        shape = (e.B, h, w, e.K) if e.dims == 2 else (e.B, d, h, w, e.K)
        x = e.bufs["x"][..., 0]
        # (several output classes: class 0 is logged)
        return _summary_arrays(x, e.target.view(shape)[..., 0], e.prob.view(shape)[..., 0], n)

    @torch.no_grad()
    def eval_sums(self, x, y) -> torch.Tensor:
        e = self.engine
        if x.shape[0] != e.B:
            raise ValueError("native eval batch must equal the per-rank batch")
        self._evaluate(x, y)
        return e.sums.clone()

    def _evaluate(self, x, y) -> None:
        """One evaluation of the full batch (x, y): the plain forward, or with --eval_tta the
        executor's `evaluate_tta` (the mean over the transforms; `sums` are then the mean's)."""
        e = self.engine
        self._pp_thr = None
        if self.tta:
            e.evaluate_tta(x, y, self.tta)
        else:
            e.load_batch(x, y)
            e.evaluate_batch()

    def _post(self, threshold: float) -> bool:
        """With --eval_components: make `prob_pp` the filter of the executor's probabilities at
        `threshold` (one `components` op per forward and threshold).  Returns whether the
        per-case ops score `prob_pp`."""
        if self.components is None:
            return False
        if self._pp_thr != threshold:
            self.engine.components(threshold, *self.components)
            self._pp_thr = threshold
        return True

    @torch.no_grad()
    def last_eval_stats(self, threshold: float = 0.5) -> torch.Tensor:
        """[B][K][6] of the batch the last ``eval_sums`` scored: one more launch on the
        probabilities and target the executor still holds."""
        return self.engine.case_stats(threshold, post=self._post(threshold)).clone()

    @torch.no_grad()
    def eval_stats(self, x, y, threshold: float = 0.5) -> torch.Tensor:
        """[n][K][6] = {I, St, Sp, TP, FP, FN} per (sample, class) of the n <= B samples given.
        A short batch is zero-padded to the per-rank batch: evaluation normalises with the
        moving BatchNorm statistics or per sample (GroupNorm), so the padding cannot change
        a real sample's result."""
        n = self._eval_padded(x, y, "eval_stats")
        return self.engine.case_stats(threshold, post=self._post(threshold))[:n].clone()

    def _eval_padded(self, x, y, what: str) -> int:
        """Evaluation forward of n <= B samples zero-padded to the per-rank batch; returns n."""
        e = self.engine
        n = x.shape[0]
        if not 1 <= n <= e.B:
            raise ValueError("native %s takes 1..%d samples (the per-rank batch), got %d" % (what, e.B, n))
        x, y = x.to(e.device).float(), y.to(e.device).float()
        if n < e.B:
            x = torch.cat([x, x.new_zeros((e.B - n,) + tuple(x.shape[1:]))])
            y = torch.cat([y, y.new_zeros((e.B - n,) + tuple(y.shape[1:]))])
        self._evaluate(x.contiguous(), y.contiguous())
        return n

    @torch.no_grad()
    def last_eval_surface(self, threshold: float = 0.5) -> torch.Tensor:
        """int32 [B][K][4] = {mp, mt, q_lo, q_hi} of the batch the last ``eval_sums`` scored
        (surf_dist.h on the probabilities and target the executor still holds)."""
        return self.engine.case_surface(threshold, post=self._post(threshold)).clone()

    @torch.no_grad()
    def eval_surface(self, x, y, threshold: float = 0.5) -> torch.Tensor:
        """int32 [n][K][4] per (sample, class) of the n <= B samples given; a short batch is
        zero-padded like ``eval_stats``."""
        n = self._eval_padded(x, y, "eval_surface")
        return self.engine.case_surface(threshold, post=self._post(threshold))[:n].clone()

    @torch.no_grad()
    def last_eval_components(self, threshold: float = 0.5) -> torch.Tensor:
        """int32 [B][K][4] = {components, kept components, largest size, kept voxels} of the
        batch the last ``eval_sums`` scored (--eval_components; components.h)."""
        _need_policy(self)
        self._post(threshold)
        return self.engine.components_info.clone()

    @torch.no_grad()
    def eval_components(self, x, y=None, threshold: float = 0.5) -> torch.Tensor:
        """int32 [n][K][4] per (sample, class) of the n <= B samples given (y is not used); a
        short batch is zero-padded like ``eval_stats``."""
        _need_policy(self)
        if y is None:
            y = torch.zeros(x.shape[:-1] + (self.spec.n_cl_out,), device=x.device)
        n = self._eval_padded(x, y, "eval_components")
        self._post(threshold)
        return self.engine.components_info[:n].clone()

    @torch.no_grad()
    def predict(self, x) -> torch.Tensor:
        e = self.engine
        self._evaluate(x, torch.zeros(x.shape[:-1] + (self.spec.n_cl_out,), device=x.device))
        if self._post(getattr(self.cfg, "eval_threshold", 0.5)):       # --eval_components: the filtered map
            return e.probs_pp().clone()
        return e.probs().clone()

    @torch.no_grad()
    def predict_sliding(self, x, overlap: float = 0.5, blend: str = "gaussian", post: bool = True) -> torch.Tensor:
        """Probabilities fp32 [n, (D,) H, W, K] of images of any spatial size, on the device: the
        executor's sliding-window path (`ExecutorBase.predict_sliding`: sw_extract, the
        evaluation forward -- with --eval_tta the mean over the transforms -- and sw_blend per
        batch of tiles, then sw_finish).  The executor's buffer, overwritten by the next call.
        post=False: the blended map itself, before the --eval_components filter."""
        self._pp_thr = None                   # (the tiles' forwards overwrite the executor's prob)
        p = self.engine.predict_sliding(x.to(self.engine.device), overlap, blend, self.tta)
        return self._sw_filter(p, getattr(self.cfg, "eval_threshold", 0.5))[0] if post else p

    def _sw_filter(self, p, threshold: float):
        """(p, None) with the filter off, else (filtered p, info) of a full-size map
        (`executor_base.sliding_components`); the last result is kept and a map that is itself
        that result is not filtered again."""
        if self.components is None:
            return p, None
        c = self._sw_pp
        if c is not None and c[1] == threshold and c[2] is p:
            return c[2], c[3]
        from .executor_base import sliding_components
        out, info = sliding_components(self.engine.C, p, threshold, *self.components)
        self._sw_pp = (None, threshold, out, info)
        return out, info

    @torch.no_grad()
    def sliding_filter(self, p, threshold: float = 0.5) -> torch.Tensor:
        """The --eval_components filter of full-size probabilities p (p itself with the flag
        off): what `predict_sliding` returns, from its post=False map."""
        return self._sw_filter(p, threshold)[0]

    @torch.no_grad()
    def sliding_components(self, p, threshold: float = 0.5) -> torch.Tensor:
        """int32 [n][K][4] of full-size probabilities p (`predict_sliding`'s result)."""
        _need_policy(self)
        return self._sw_filter(p, threshold)[1]

    @torch.no_grad()
    def sliding_stats(self, p, y, threshold: float = 0.5, post: bool = True) -> torch.Tensor:
        """fp32 [n][K][6] of full-size probabilities p (`predict_sliding`) against the target y.
        post=False: of p itself, the --eval_components filter not applied."""
        from .executor_base import sliding_stats
        return sliding_stats(self.engine.C, self._sw_filter(p, threshold)[0] if post else p, y, threshold)

    @torch.no_grad()
    def sliding_surface(self, p, y, threshold: float = 0.5, post: bool = True) -> torch.Tensor:
        """int32 [n][K][4] of full-size probabilities p (`predict_sliding`) against the target y.
        post=False: of p itself, the --eval_components filter not applied."""
        from .executor_base import sliding_surface
        return sliding_surface(self.engine.C, self._sw_filter(p, threshold)[0] if post else p, y, threshold)

    @torch.no_grad()
    def filter_once(self, p, threshold: float = 0.5):
        """(filtered p, info or None) of the --eval_components filter, the kept last result neither
        used nor replaced (`Predictor.segment`: a case's map is filtered under another shape)."""
        if self.components is None:
            return p, None
        from .executor_base import sliding_components
        return sliding_components(self.engine.C, p, threshold, *self.components)

    @torch.no_grad()
    def sliding_labels(self, p, threshold: float = 0.5, rule: str = "nested", values=(1,), out_shape=None,
                       offset=(0, 0, 0)):
        """(labels uint8, counts int32 [n][K + 1]) on the device of full-size probabilities p: the
        `labelmap` op (`executor_base.sliding_labels`)."""
        from .executor_base import sliding_labels
        return sliding_labels(self.engine.C, p, threshold, rule, values, out_shape, offset)

    def adam_step(self, lr, b1p, b2p, grad_scale=1.0):
        self.engine.adam_step(lr, b1p, b2p, grad_scale)


def _policy(cfg):
    """(keep_largest, min_size) of cfg.eval_components, or None with the flag off."""
    s = str(getattr(cfg, "eval_components", "") or "")
    return parse_components(s) if s.strip() else None


def _need_policy(backend) -> None:
    if backend.components is None:
        raise RuntimeError("no component policy: build the backend with --eval_components (largest, min:V)")


def _summary_arrays(x, t, p, n) -> dict:
    def prep(a):
        a = a[:n].detach().float()
        if a.dim() == 5:                     # [n, D, H, W, 1]
            a = a[..., 0]
        if a.dim() == 4 and a.shape[-1] == 1:
            a = a[..., 0]
        if a.dim() == 4:                     # 3D volume [n, D, H, W]: middle slice
            a = a[:, a.shape[1] // 2]
        return a.cpu().numpy()
    if x.dim() == 4 and x.shape[-1] > 1 and t.dim() == 4 and t.shape[-1] == 1:
        x = x[..., 0]                        # NHWC input: first channel
    elif x.dim() == 5 and x.shape[-1] > 1:
        x = x[..., 0]
    return {"predictions": prep(p), "ground_truth": prep(t), "images": prep(x)}


def native_supported(spec, cfg, device) -> Optional[str]:
    """None if the native executor supports this config, else the reason."""
    if torch.device(device).type != "cuda":
        return "not on a GPU"
    if cfg.dtype not in ("bf16", "fp16", "fp32"):
        return "native kernels are bf16 / fp16 / fp32 (dtype=%s)" % cfg.dtype
    if not 1 <= spec.n_cl_out <= 4:
        return "n_cl_out=%d: the head kernels take 1..4 output classes" % spec.n_cl_out
    if spec.n_cl_out > 1:
        # the multi-class head (csrc/kernels/head_mc.hip) is the unfused 16-bit head
        if spec.norm != "none":
            return ("n_cl_out=%d with norm=%s: the normalised head kernels are single-class"
                    % (spec.n_cl_out, spec.norm))
        if cfg.dtype == "fp32":
            return "n_cl_out=%d with dtype=fp32: the fp32 executor's head is single-class" % spec.n_cl_out
    if cfg.dtype == "fp32":
        # (runtime/f32_engine.py: the reference's own configuration family)
        if spec.norm != "none":
            return "the fp32 executor runs the reference's norm-free model (norm=%s: use bf16 / fp16)" % spec.norm
        if spec.base not in (16, 32, 64):
            return "fp32 head input channels must be 16, 32 or 64 (base %d)" % spec.base
        return None
    if spec.base not in (32, 64):
        # the fused head / head kernels take 16, 32 or 64 head-input channels and the
        # row-window kernels 32-channel chunks
        return "base filters must be 32 or 64 (got %d)" % spec.base
    cin = spec.in_channels
    if not (cin <= 8 or cin % 32 == 0):
        return "in_channels=%d" % cin
    return None


def resolve_backend(want: str, spec, cfg, device) -> str:
    """'native' or 'torch' for a requested ``--backend`` (auto / native / torch).

    One GPU path: on a GPU, ``auto`` means the HIP executor and a
    config it does not support is an error with the reason -- never a silent ATen /
    MIOpen run.  ATen stays reachable only by asking for it (``--backend torch``: the
    numerical oracle and baseline) and is what ``auto`` means off the GPU (the CPU /
    gloo plumbing config)."""
    if want == "torch":
        return "torch"
    reason = native_supported(spec, cfg, device)
    on_gpu = torch.device(device).type == "cuda"
    if want == "native" or (want == "auto" and on_gpu):
        if reason is not None:
            raise RuntimeError("the native HIP executor does not support this config (%s); "
                               "pass --backend torch to run the ATen reference path explicitly" % reason)
        return "native"
    return "torch"


def make_backend(spec, flat, cfg, device, per_rank_batch, bounds=None):
    if resolve_backend(cfg.backend, spec, cfg, device) == "native":
        from .. import native
        native.require()
        return NativeBackend(spec, flat, cfg, device, per_rank_batch, bounds)
    return TorchBackend(spec, flat, cfg, device, per_rank_batch, bounds)

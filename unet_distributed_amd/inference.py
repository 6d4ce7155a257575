"""Inference on an exported model (the reference's ``tf.saved_model.loader``
flow, `sanity_check_trained_model.py:38-44`).

:func:`load_saved_model` reads ``saved_model/saved_model.pb`` -- the ``serve`` tag, the
``intel_unet_brats_model`` signature's input / output tensors (``Placeholder:0`` ->
``Mask/Sigmoid:0``) and the UNet architecture recovered from the GraphDef
(:func:`utils.tf_graph.spec_from_graph`: VariableV2 shapes, pool / upsample / norm
nodes) -- and the weights from ``saved_model/variables/variables.{index,data-*}`` (TF
bundle), both written by :func:`utils.checkpoint.export_model`; the JSON side-car is
only a fallback for directories without a ``saved_model.pb``.  It returns a
:class:`Predictor` whose ``predict(x)`` maps NHWC(/NDHWC) float images to sigmoid
probabilities.

On a GPU the native HIP executor's inference plan runs (forward only, dropout
off, fused head+sigmoid) at a fixed micro-batch; a short last batch is padded.
Elsewhere, or for configs the native executor does not cover, the ATen
reference forward runs.  ``predict`` takes images of the model's input size;
``predict_sliding`` / ``stats_sliding`` / ``surface_sliding`` take images of any spatial
size (sliding-window inference, :mod:`unet_distributed_amd.ops.sliding`).
"""

import json
import os
from typing import Optional

import numpy as np
import torch

from .models.spec import UNetSpec
from .runtime.params import FlatParams
from .utils import tf_bundle
from .utils.checkpoint import tensors_to_flat


class _Cfg:
    """Minimal config for the backends (inference needs no optimiser flags)."""

    def __init__(self, img_size, dtype, eval_dropout=False, eval_tta="", eval_components=""):
        self.eval_tta = eval_tta
        self.eval_components = eval_components
        self.eval_threshold = 0.5
        self.img_size = img_size
        self.dtype = dtype
        self.loss = "dice"
        self.bce_weight = 1.0
        self.eval_dropout = eval_dropout
        self.backend = "auto"


class Predictor:
    def __init__(self, spec: UNetSpec, flat: FlatParams, img_size: int, device, batch: int,
                 dtype: str = "bf16", backend: str = "auto", state=None, tta: str = "", components: str = ""):
        """`tta`: test-time augmentation, a comma list of flip and rot90 (the --eval_tta
        spelling): `predict`, `stats` and `surface` then score the mean over the transforms.
        `components`: connected-component filter, a comma list of largest and min:V (the
        --eval_components spelling): `predict` / `predict_sliding` then return the filtered
        map (thresholded at 0.5), `stats` and `surface` score it and `components` /
        `components_sliding` give the component counts."""
        from .config import parse_components, parse_tta
        from .runtime.backends import NativeBackend, TorchBackend, resolve_backend
        self.spec, self.flat, self.batch, self.img_size = spec, flat, batch, img_size
        self.device = torch.device(device)
        parse_tta(tta)
        parse_components(components)
        cfg = _Cfg(img_size, dtype if self.device.type == "cuda" else "fp32", eval_tta=tta,
                   eval_components=components)
        if resolve_backend(backend, spec, cfg, self.device) == "native":
            from . import native
            native.require()
            self.backend = NativeBackend(spec, flat, cfg, self.device, batch)
            self.backend.engine.repack()
        else:
            self.backend = TorchBackend(spec, flat, cfg, self.device, batch)
        # BatchNorm moving statistics (both backends keep them under the same names;
        # the native inference plan normalises with them)
        for k, v in (state or {}).items():
            if k in self.backend.state:
                self.backend.state[k].copy_(torch.as_tensor(np.asarray(v, np.float32)))
        self.name = self.backend.name

    @torch.no_grad()
    def predict(self, x) -> np.ndarray:
        """Probabilities for a batch of any length (native: chunks of ``batch``)."""
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        n = x.shape[0]
        if self.backend.name != "native":
            return self.backend.predict(x.to(self.device)).float().cpu().numpy()
        outs = []
        for s in range(0, n, self.batch):
            xb = x[s:s + self.batch]
            m = xb.shape[0]
            if m < self.batch:
                xb = torch.cat([xb, xb.new_zeros((self.batch - m,) + tuple(xb.shape[1:]))])
            p = self.backend.predict(xb.to(self.device))
            outs.append(p[:m].float().cpu())
        return torch.cat(outs).numpy()

    @torch.no_grad()
    def stats(self, x, y, threshold: float = 0.5) -> np.ndarray:
        """``[n][K][6] = {I, St, Sp, TP, FP, FN}`` per (sample, class) for any n
        (``ops.seg_metrics``; native: chunks of ``batch``, a short last chunk padded)."""
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
        if self.backend.name != "native":
            return self.backend.eval_stats(x.to(self.device), y.to(self.device), threshold).cpu().numpy()
        outs = [self.backend.eval_stats(x[s:s + self.batch].to(self.device), y[s:s + self.batch].to(self.device),
                                        threshold).double().cpu() for s in range(0, x.shape[0], self.batch)]
        return torch.cat(outs).numpy()

    @torch.no_grad()
    def surface(self, x, y, threshold: float = 0.5) -> np.ndarray:
        """int64 ``[n][K][4] = {mp, mt, q_lo, q_hi}`` per (sample, class) for any n: the
        surface-distance integers of HD95 (``ops.seg_metrics.hd95_from_surface``; native:
        chunks of ``batch``, a short last chunk padded)."""
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
        step = self.batch if self.backend.name == "native" else max(1, x.shape[0])
        outs = [self.backend.eval_surface(x[s:s + step].to(self.device), y[s:s + step].to(self.device),
                                          threshold).long().cpu() for s in range(0, x.shape[0], step)]
        return torch.cat(outs).numpy()

    @torch.no_grad()
    def components(self, x, threshold: float = 0.5) -> np.ndarray:
        """int64 ``[n][K][4] = {components, kept components, largest size, kept voxels}`` per
        (sample, class) for any n, of the `components=` policy (``ops.components``; native:
        chunks of ``batch``, a short last chunk padded)."""
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        step = self.batch if self.backend.name == "native" else max(1, x.shape[0])
        outs = [self.backend.eval_components(x[s:s + step].to(self.device), None, threshold).long().cpu()
                for s in range(0, x.shape[0], step)]
        return torch.cat(outs).numpy()

    # ------------------------------------------------------------------ images of any spatial size
    def sliding_chunks(self, shape, max_bytes: int = 1 << 30):
        """[(begin, end)] of the chunks of whole images that `predict_sliding` works in: as many
        images [(D,) H, W, Cin] as keep a chunk's fp32 input and accumulator (Cin + K floats per
        pixel) under `max_bytes`, at least one.  Tile numbering restarts per chunk."""
        if len(shape) != self.spec.dims + 2 or shape[-1] != self.spec.in_channels:
            raise ValueError("sliding window: images [n, %sH, W, %d], got shape %r"
                             % ("D, " if self.spec.dims == 3 else "", self.spec.in_channels, tuple(shape)))
        per = int(np.prod(shape[1:-1])) * (self.spec.in_channels + self.spec.n_cl_out) * 4
        m = max(1, int(max_bytes) // per)
        return [(s, min(shape[0], s + m)) for s in range(0, shape[0], m)]

    def _sliding(self, x, overlap, blend, max_bytes, score):
        from .ops import sliding
        sliding.check_overlap(overlap)
        sliding.check_blend(blend)
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        outs = []
        for s, t in self.sliding_chunks(tuple(x.shape), max_bytes):
            outs.append(score(self.backend.predict_sliding(x[s:t].to(self.device), overlap, blend), s, t).cpu())
        return torch.cat(outs).numpy()

    @torch.no_grad()
    def predict_sliding(self, x, overlap: float = 0.5, blend: str = "gaussian", max_bytes: int = 1 << 30) -> np.ndarray:
        """Probabilities fp32 [n, (D,) H, W, K] of images x [n, (D,) H, W, Cin] of any spatial size
        by sliding-window inference (`ops.sliding`): overlapping tiles of the model's size at
        stride T - floor(overlap T), every tile through the forward (with `tta=` the mean over
        the transforms), blended with `blend` weights (constant | gaussian) and divided by the
        summed weights.  Native: tile extraction and blend are HIP kernels (kernels/sliding.h)."""
        return self._sliding(x, overlap, blend, max_bytes, lambda p, s, t: p.float())

    @torch.no_grad()
    def stats_sliding(self, x, y, threshold: float = 0.5, overlap: float = 0.5, blend: str = "gaussian",
                      max_bytes: int = 1 << 30) -> np.ndarray:
        """``[n][K][6] = {I, St, Sp, TP, FP, FN}`` per (image, class) of `predict_sliding`'s
        probabilities against the full-size target y [n, (D,) H, W, K]."""
        y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
        return self._sliding(x, overlap, blend, max_bytes, lambda p, s, t: self.backend.sliding_stats(
            p, y[s:t].to(self.device), threshold).double())

    @torch.no_grad()
    def surface_sliding(self, x, y, threshold: float = 0.5, overlap: float = 0.5, blend: str = "gaussian",
                        max_bytes: int = 1 << 30) -> np.ndarray:
        """int64 ``[n][K][4] = {mp, mt, q_lo, q_hi}`` per (image, class) of `predict_sliding`'s
        probabilities against the full-size target y: the surface-distance integers of HD95."""
        y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
        return self._sliding(x, overlap, blend, max_bytes, lambda p, s, t: self.backend.sliding_surface(
            p, y[s:t].to(self.device), threshold).long())


    @torch.no_grad()
    def components_sliding(self, x, threshold: float = 0.5, overlap: float = 0.5, blend: str = "gaussian",
                           max_bytes: int = 1 << 30) -> np.ndarray:
        """int64 ``[n][K][4]`` per (image, class) of the `components=` policy on `predict_sliding`'s
        blended full-size probabilities."""
        return self._sliding(x, overlap, blend, max_bytes, lambda p, s, t: self.backend.sliding_components(
            p, threshold).long())

    @torch.no_grad()
    def segment(self, x, threshold: float = 0.5, labels: str = "", overlap: float = 0.5, blend: str = "gaussian",
                volume: bool = False, out_shape=None, offset=None, max_bytes: int = 1 << 30, mode=None,
                visit=None):
        """(labels uint8 ndarray, counts int64 ndarray) of images x [n, (D,) H, W, Cin] of any
        spatial size: `predict_sliding`'s blended probabilities, the `components=` filter if the
        Predictor has one, then the label map of `ops.labelmap` under the rule and values of
        `labels` (the --labels spelling; `mode` picks its defaults) -- all on the device (native:
        the `labelmap` kernel), so only the uint8 labels are copied to the host.

        volume=False: the images are independent; labels [n, (Do,) Ho, Wo], counts [n][K + 1].
        volume=True (2D models): the n slices are one case, filtered 6-connected as the volume
        [1, n, H, W, K]; labels [n, Ho, Wo], counts [1][K + 1].  `out_shape` / `offset`: the label
        map is pasted at `offset` into a zero destination of `out_shape` ((H, W) pairs, or
        (D, H, W) triples); None is the source's own shape.  `visit(p, info, s, t)`, if given, is
        called with the filtered probabilities of the images [s, t) on the device ([1, n, H, W, K]
        of the whole case with volume=True) and the filter's info (None with the filter off)."""
        from .ops import labelmap, sliding
        sliding.check_overlap(overlap)
        sliding.check_blend(blend)
        K = self.spec.n_cl_out
        rule, values = labelmap.parse_labels(labels, K, mode)
        if volume and self.spec.dims != 2:
            raise ValueError("segment: volume=True joins the slices of a 2D model; a 3D model's image is a volume")
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        be = self.backend
        off = (0, 0, 0) if offset is None else tuple(offset)
        chunks = self.sliding_chunks(tuple(x.shape), max_bytes)
        if volume:
            n = x.shape[0]
            joined = None
            for s, t in chunks:
                p = be.predict_sliding(x[s:t].to(self.device), overlap, blend, post=False)
                if joined is None:
                    joined = torch.empty((n,) + tuple(p.shape[1:]), dtype=torch.float32, device=p.device)
                joined[s:t].copy_(p)          # (the backend's buffer is overwritten by the next chunk)
            case, info = be.filter_once(joined.unsqueeze(0), threshold)
            if visit is not None:
                visit(case, info, 0, n)
            if out_shape is not None and len(out_shape) == 2:
                out_shape = (n,) + tuple(out_shape)
            off = (0,) + off if len(off) == 2 else off
            lab, counts = be.sliding_labels(case, threshold, rule, values, out_shape, off)
            return lab[0].cpu().numpy(), counts.long().cpu().numpy()
        labs, cnts = [], []
        for s, t in chunks:
            p = be.predict_sliding(x[s:t].to(self.device), overlap, blend, post=False)
            p, info = be.filter_once(p, threshold)
            if visit is not None:
                visit(p, info, s, t)
            lab, counts = be.sliding_labels(p, threshold, rule, values, out_shape, off)
            labs.append(lab.cpu())
            cnts.append(counts.long().cpu())
        return torch.cat(labs).numpy(), torch.cat(cnts).numpy()


SIGNATURE ="intel_unet_brats_model"


def _spec_from_pb(path: str):
    from .utils import tf_graph
    sm = tf_graph.read_saved_model(path)
    if "serve" not in sm["tags"]:
        raise ValueError("%s has no 'serve' meta graph" % path)
    if SIGNATURE not in sm["signatures"]:
        raise ValueError("%s has no %s signature" % (path, SIGNATURE))
    sig = sm["signatures"][SIGNATURE]
    if sig["inputs"]["image"]["name"] != "Placeholder:0" or sig["outputs"]["prediction"]["name"] != "Mask/Sigmoid:0":
        raise ValueError("unexpected signature tensors %s" % sig)
    return tf_graph.spec_from_graph(sm, SIGNATURE)


def _spec_from_json(path: str):
    with open(path) as f:
        meta = json.load(f)
    if "serve" not in meta.get("tags", []):
        raise ValueError("export %s has no 'serve' tag" % path)
    m = meta["model"]
    spec = UNetSpec(in_channels=m["in_channels"], n_cl_out=m["n_cl_out"], base=m["base"], depth=m["depth"],
                    use_upsampling=m["use_upsampling"], dims=m["dims"], dropout=m["dropout"],
                    norm=m.get("norm", "none"), groups=m.get("groups", 8))
    sig = next(iter(meta["signature_def"].values()))
    return spec, meta.get("img_size") or sig["inputs"]["image"]["shape"][1]


def load_saved_model(export_dir: str, device=None, batch: int = 128, dtype: str = "bf16",
                     backend: str = "auto", tta: str = "", components: str = "") -> Predictor:
    pb = os.path.join(export_dir, "saved_model.pb")
    if os.path.exists(pb):
        spec, img_size = _spec_from_pb(pb)
    else:
        spec, img_size = _spec_from_json(os.path.join(export_dir, "saved_model.json"))
    if device is None:
        device = "cuda:0" if torch.cuda.is_available() else "cpu"
    flat = FlatParams(spec, device=device)
    tensors = tf_bundle.read_bundle(os.path.join(export_dir, "variables", "variables"))
    tensors_to_flat(flat, tensors, strict=True)
    state = {k: v for k, v in tensors.items() if k.endswith("moving_mean") or k.endswith("moving_variance")}
    return Predictor(spec, flat, int(img_size), device, batch, dtype=dtype, backend=backend, state=state,
                     tta=tta, components=components)

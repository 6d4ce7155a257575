"""Case-level prediction with an exported model: scans in, label-map files out.

``predict.py --export_dir <dir> --out_dir <dir>`` plus one source of images:

* ``--case_dir <BraTS case> ...`` / ``--cases_dir <dir of cases>``: the modality volumes of a
  case folder (:mod:`unet_distributed_amd.data.preprocess`: the same files, crop and z-score
  as training) go through :meth:`inference.Predictor.segment` -- sliding windows over the
  whole slice by default, the ``--components`` filter, the label map of
  :mod:`unet_distributed_amd.ops.labelmap` -- and ``<out_dir>/<case>.mha`` holds the uint8
  label volume (z, y, x) in the geometry, spacing and origin of the first modality found.  A
  2D model takes the case's slices as one volume (the filter is 6-connected over the case), a
  3D model takes the case as one image.  With ``--img_rows`` / ``--img_cols`` the centre crop
  of training is predicted and pasted back at the crop's lower margins.
* ``--data_path <npy dir>`` (``imgs_test.npy``) / ``--synthetic N``: independent images,
  ``labels_test.npy`` / ``labels_synthetic.npy`` uint8 ``[n, (D,) H, W]``.

One JSON record per case (or per image set) is appended to ``<out_dir>/predictions.jsonl``.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

from . import settings
from .data import datasets


def _voxels(labels: np.ndarray, counts: np.ndarray, values) -> dict:
    """{label value: voxels} of a label array from the slot counts of its source voxels: the
    background is everything else (slot 0 and the padding around a pasted crop)."""
    per = counts.reshape(-1, counts.shape[-1]).sum(0)
    v = {str(int(val)): int(per[m + 1]) for m, val in enumerate(values)}
    v["0"] = int(labels.size) - sum(v.values())
    return v


def _score(model, p, y, threshold, hd95):
    """Per-region Dice, sensitivity, specificity (and HD95) of filtered probabilities p
    against the truth regions y, both [n, (D,) H, W, K]: `ops.seg_metrics`' conventions."""
    import torch
    yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32)).to(p.device)
    out = {"stats": model.backend.sliding_stats(p, yt, threshold, post=False).double().cpu().numpy(),
           "grid": tuple(p.shape[1:-1])}
    if hd95:
        out["surf"] = model.backend.sliding_surface(p, yt, threshold, post=False).long().cpu().numpy()
    return out


def _score_record(parts) -> dict:
    """The `score` entry of a record from the `_score` results of its images."""
    from .ops import seg_metrics
    grid = parts[0]["grid"]
    m = seg_metrics.metrics_from_case_stats(np.concatenate([q["stats"] for q in parts]), int(np.prod(grid)))
    rec = {"dice": m["case_dice"], "sensitivity": m["sensitivity"], "specificity": m["specificity"],
           "cases": m["cases"]}
    if "surf" in parts[0]:
        h = seg_metrics.hd95_metrics(seg_metrics.accumulate_hd95(np.concatenate([q["surf"] for q in parts]), grid))
        rec["hd95"] = h["hd95"]
    return seg_metrics.jsonable(rec)


def predict_case(model, case_dir: str, a, out_dir: str) -> dict:
    """Predict one BraTS case folder, write ``<out_dir>/<case>.mha`` and return its record."""
    from .data import preprocess
    from .data.mha import read_mha, write_mha
    from .ops import labelmap
    name = os.path.basename(os.path.normpath(case_dir))
    files, truth, _ = preprocess.find_case_files(case_dir)
    first = next((files[s] for s in preprocess.SERIES if s in files), None)
    if first is None:
        raise SystemExit("predict: no modality volume (MR_T1 / MR_T1c / MR_Flair / MR_T2) found in %s" % case_dir)
    ref = read_mha(first)
    Z, Y, X = ref.array.shape
    rows, cols = a.img_rows or X, a.img_cols or Y          # (rows: the x extent, as `crop_shrink`)
    if rows > X or cols > Y:
        raise SystemExit("predict: the crop %d x %d is larger than the slices %d x %d of %s" % (rows, cols, X, Y, name))
    img, lab, _ = preprocess.case_arrays(case_dir, rows, cols, 1)
    lx, ly = (X - rows) // 2, (Y - cols) // 2
    K, dims = model.spec.n_cl_out, model.spec.dims
    x = datasets.select_images(img, model.spec.in_channels if a.in_channels is None else a.in_channels, a.mode)
    scored, info_box = [], []

    def visit(p, info, s, t):
        if info is not None:
            info_box.append(info.long().cpu().numpy())
        if a.score and truth is not None:
            y = datasets.select_masks(lab, K, a.mode)
            scored.append(_score(model, p, y[None], a.threshold, a.hd95))

    kw = dict(threshold=a.threshold, labels=a.labels, overlap=a.overlap, blend=a.blend, mode=a.mode, visit=visit)
    t0 = time.time()
    if dims == 2:
        labels, counts = model.segment(x, volume=True, out_shape=(Y, X), offset=(ly, lx), **kw)
    else:
        labels, counts = model.segment(x[None], out_shape=(Z, Y, X), offset=(0, ly, lx), **kw)
        labels = labels[0]
    dt = time.time() - t0
    write_mha(os.path.join(out_dir, name + ".mha"), labels, spacing=ref.spacing, origin=ref.origin,
              compress=a.compress)
    _, values = labelmap.parse_labels(a.labels, K, a.mode)
    vox = _voxels(labels, counts, values)
    ml = float(np.prod(ref.spacing)) / 1000.0
    rec = {"name": name, "shape": [int(v) for v in labels.shape], "voxels": vox,
           "volume_ml": {k: v * ml for k, v in vox.items() if k != "0"}, "seconds": dt, "backend": model.name}
    if info_box:
        info = np.concatenate(info_box)
        rec["components"] = {"before": [int(v) for v in info[..., 0].sum(0)],
                             "after": [int(v) for v in info[..., 1].sum(0)]}
    if a.score:
        rec["scored"] = bool(scored)
        if scored:
            rec["score"] = _score_record(scored)
    return rec


def predict_images(model, x, y, tag: str, a, out_dir: str) -> dict:
    """Predict independent images x, write ``labels_<tag>.npy`` and return the summary record."""
    from .ops import labelmap
    K = model.spec.n_cl_out
    scored, info_box = [], []

    def visit(p, info, s, t):
        if info is not None:
            info_box.append(info.long().cpu().numpy())
        if a.score and y is not None:
            scored.append(_score(model, p, np.asarray(y[s:t], dtype=np.float32), a.threshold, a.hd95))

    t0 = time.time()
    labels, counts = model.segment(np.asarray(x, dtype=np.float32), threshold=a.threshold, labels=a.labels,
                                   overlap=a.overlap, blend=a.blend, mode=a.mode, visit=visit)
    dt = time.time() - t0
    np.save(os.path.join(out_dir, "labels_%s.npy" % tag), labels)
    _, values = labelmap.parse_labels(a.labels, K, a.mode)
    rec = {"name": tag, "shape": [int(v) for v in labels.shape], "voxels": _voxels(labels, counts, values),
           "seconds": dt, "backend": model.name}
    if info_box:
        info = np.concatenate(info_box)
        rec["components"] = {"before": [int(v) for v in info[..., 0].sum(0)],
                             "after": [int(v) for v in info[..., 1].sum(0)]}
    if a.score:
        rec["scored"] = bool(scored)
        if scored:
            rec["score"] = _score_record(scored)
    return rec


def main(argv=None) -> list:
    p = argparse.ArgumentParser(description="Label-map files from scans with an exported model")
    p.add_argument("--export_dir", default=os.path.join(settings.CHECKPOINT_DIRECTORY, "saved_model"))
    p.add_argument("--out_dir", required=True)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--case_dir", nargs="+", metavar="DIR", help="BraTS case folders (sub-folders of .mha volumes)")
    src.add_argument("--cases_dir", metavar="DIR", help="a folder of BraTS case folders")
    src.add_argument("--data_path", metavar="DIR", help="a folder with imgs_test.npy (and msks_test.npy for --score)")
    src.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic test images")
    p.add_argument("--synthetic_size", type=int, default=0, metavar="S",
                   help="side of the --synthetic images (default: the model's input size)")
    p.add_argument("--mode", type=int, default=settings.MODE)
    p.add_argument("--in_channels", type=int, default=None, help="default: the model's input channels")
    p.add_argument("--img_rows", type=int, default=0, help="centre crop of a case's slices (0: the whole slice)")
    p.add_argument("--img_cols", type=int, default=0)
    p.add_argument("--rescale_factor", type=int, default=1)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--labels", default="", metavar="SPEC",
                   help="<rule>[:v1,v2,..]: rule nested | argmax and the label values of the output channels "
                        "(default nested; values 1..K, or 2,1,4 for three channels in --mode 5)")
    p.add_argument("--components", default="", metavar="SPEC",
                   help="connected-component filter of the thresholded prediction: a comma list of largest and / "
                        "or min:V (voxels); over the whole case for BraTS cases")
    p.add_argument("--tta", default="", metavar="SPEC", help="test-time augmentation: flip and / or rot90")
    p.add_argument("--overlap", type=float, default=0.5, metavar="F")
    p.add_argument("--blend", default="gaussian", choices=["constant", "gaussian"])
    p.add_argument("--batch_size", type=int, default=128, help="tiles per forward")
    p.add_argument("--backend", default="auto", choices=["auto", "native", "torch"])
    p.add_argument("--device", default=None)
    p.add_argument("--compress", action="store_true", help="zlib-compressed .mha files")
    p.add_argument("--score", action="store_true",
                   help="where a ground truth exists: per-region Dice, sensitivity and specificity in the record")
    p.add_argument("--hd95", action="store_true", help="--score: also the 95th-percentile Hausdorff distance")
    a = p.parse_args(argv)
    if a.rescale_factor != 1:
        raise SystemExit("--rescale_factor %d: prediction works at the scans' own resolution (there is no label "
                         "upsampling); use 1" % a.rescale_factor)
    if not 0.0 <= a.overlap <= 0.75:
        raise SystemExit("--overlap must lie in [0, 0.75], got %r" % a.overlap)
    if not 0.0 < a.threshold < 1.0:
        raise SystemExit("--threshold must lie strictly inside (0, 1), got %r" % a.threshold)
    from .inference import load_saved_model
    from .ops import labelmap
    print("Loading trained model from directory {}".format(a.export_dir))
    model = load_saved_model(a.export_dir, device=a.device, batch=a.batch_size, backend=a.backend, tta=a.tta,
                             components=a.components)
    K = model.spec.n_cl_out
    print("Labels: %s" % labelmap.describe(*labelmap.parse_labels(a.labels, K, a.mode)))
    if a.components.strip():
        from .ops.components import describe
        print("Evaluation components: %s" % describe(a.components))
    os.makedirs(a.out_dir, exist_ok=True)
    records = []
    if a.case_dir or a.cases_dir:
        cases = list(a.case_dir or [])
        if a.cases_dir:
            cases = [os.path.join(a.cases_dir, n) for n in sorted(os.listdir(a.cases_dir))
                     if os.path.isdir(os.path.join(a.cases_dir, n))]
        for d in cases:
            rec = predict_case(model, d, a, a.out_dir)
            tail = ""
            if a.score:
                tail = ", Dice = %s" % rec["score"]["dice"] if rec.get("scored") else ", unscored (no ground truth)"
            print("%s: %s voxels by label %s, %.2f s%s" % (rec["name"], "x".join(map(str, rec["shape"])),
                                                           json.dumps(rec["voxels"], sort_keys=True),
                                                           rec["seconds"], tail))
            records.append(rec)
    else:
        if a.synthetic:
            x, y = datasets.synthetic_brats(a.synthetic, a.synthetic_size or model.img_size, model.spec.in_channels,
                                            model.spec.dims, seed=1, out_channels=K)
            tag = "synthetic"
        else:
            cin = model.spec.in_channels if a.in_channels is None else a.in_channels
            x = datasets.select_images(np.load(os.path.join(a.data_path, "imgs_test.npy"), mmap_mode="r"), cin, a.mode)
            mp = os.path.join(a.data_path, "msks_test.npy")
            y = datasets.select_masks(np.load(mp, mmap_mode="r"), K, a.mode) if a.score and os.path.exists(mp) else None
            tag = "test"
        rec = predict_images(model, x, y, tag, a, a.out_dir)
        print("%s: %s voxels by label %s, %.2f s" % (tag, "x".join(map(str, rec["shape"])),
                                                     json.dumps(rec["voxels"], sort_keys=True), rec["seconds"]))
        records.append(rec)
    with open(os.path.join(a.out_dir, "predictions.jsonl"), "a") as f:
        for rec in records:
            f.write(json.dumps(rec, sort_keys=True) + "\n")
    print("({} records, {} backend) -> {}".format(len(records), model.name, a.out_dir))
    return records


if __name__ == "__main__":
    main()
    sys.exit(0)

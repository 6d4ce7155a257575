"""Post-hoc check of an exported model (`sanity_check_trained_model.py`, C22).

Loads ``<checkpoint_dir>/saved_model`` (:mod:`unet_distributed_amd.inference`),
runs it over the test set in batches of 128 and prints the average per-batch
Dice with the script's own smoothing ``2(sum(a*b)+1)/(sum(a+b)+1)``
(`sanity_check_trained_model.py:30-35`).

Batch iteration reproduces the reference exactly by default:
``range(0, n - batch_size, batch_size)`` -- which drops the last full batch
whenever ``n`` is a multiple of the batch size, and the partial tail
(`sanity_check_trained_model.py:51`).  ``--all_batches`` covers every sample
instead (fix).
"""

import argparse
import os
import sys
import time

import numpy as np

from . import settings
from .data import datasets
from .ops.losses import sanity_dice


def batch_starts(n: int, batch_size: int, all_batches: bool = False):
    if all_batches:
        return list(range(0, n, batch_size))
    return list(range(0, n - batch_size, batch_size))


def main(argv=None) -> float:
    p = argparse.ArgumentParser(description="Average test-set Dice of an exported model")
    p.add_argument("--export_dir", default=os.path.join(settings.CHECKPOINT_DIRECTORY, "saved_model"))
    p.add_argument("--data_path", default=settings.OUT_PATH)
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--in_channels", type=int, default=settings.IN_CHANNEL_NO)
    p.add_argument("--out_channels", type=int, default=settings.OUT_CHANNEL_NO)
    p.add_argument("--mode", type=int, default=settings.MODE)
    p.add_argument("--device", default=None)
    p.add_argument("--backend", default="auto", choices=["auto", "native", "torch"])
    p.add_argument("--all_batches", action="store_true")
    p.add_argument("--per_class", action="store_true",
                   help="also print per-class case Dice, sensitivity and specificity (thresholded at 0.5)")
    p.add_argument("--hd95", action="store_true",
                   help="also print the per-class 95th-percentile Hausdorff distance in voxels (thresholded at 0.5)")
    p.add_argument("--tta", default="", metavar="SPEC",
                   help="test-time augmentation: score the mean prediction over flip and / or rot90 (comma-separated)")
    p.add_argument("--components", default="", metavar="SPEC",
                   help="connected-component filter of the thresholded prediction before scoring: a comma list of "
                        "largest and / or min:V (voxels), e.g. largest,min:20")
    p.add_argument("--synthetic", type=int, default=0, metavar="N",
                   help="use N synthetic test slices instead of the .npy files")
    p.add_argument("--synthetic_size", type=int, default=0, metavar="S",
                   help="side of the --synthetic images (default: the model's input size; "
                        "another size needs --sliding)")
    p.add_argument("--sliding", action="store_true",
                   help="sliding-window inference: the test images may have any spatial size "
                        "(overlapping tiles of the model's size, blended); covers every sample, as --all_batches")
    p.add_argument("--overlap", type=float, default=0.5, metavar="F",
                   help="--sliding: fraction of a tile shared with its neighbour, 0 .. 0.75")
    p.add_argument("--blend", default="gaussian", choices=["constant", "gaussian"],
                   help="--sliding: weights of a tile's pixels in the blend")
    a = p.parse_args(argv)
    if not 0.0 <= a.overlap <= 0.75:
        p.error("--overlap must lie in [0, 0.75], got %r" % a.overlap)
    from .inference import load_saved_model
    print("Loading trained model from directory {}".format(a.export_dir))
    model = load_saved_model(a.export_dir, device=a.device, batch=a.batch_size, backend=a.backend, tta=a.tta,
                             components=a.components)
    if a.components.strip():
        from .ops.components import describe
        print("Evaluation components: %s" % describe(a.components))
    print('-' * 38)
    print('Loading and preprocessing test data...')
    print('-' * 38)
    if a.synthetic:
        if a.synthetic_size and a.synthetic_size != model.img_size and not a.sliding:
            p.error("--synthetic_size %d differs from the model's input size %d: add --sliding"
                    % (a.synthetic_size, model.img_size))
        x, y = datasets.synthetic_brats(a.synthetic, a.synthetic_size or model.img_size, model.spec.in_channels,
                                        model.spec.dims, seed=1, out_channels=model.spec.n_cl_out)
    else:
        xi, yi = datasets.load_data(a.data_path, "_test")
        x, y = datasets.update_channels(xi, yi, a.in_channels, a.out_channels, a.mode)
    # --sliding: the same loops through the sliding-window methods (images of any spatial size),
    # over every sample (the reference's iteration, which drops the tail, is kept for its own flow)
    every = a.all_batches or a.sliding
    sw = dict(overlap=a.overlap, blend=a.blend)
    predict = (lambda v: model.predict_sliding(v, **sw)) if a.sliding else model.predict
    stats_of = (lambda v, t: model.stats_sliding(v, t, **sw)) if a.sliding else model.stats
    surface_of = (lambda v, t: model.surface_sliding(v, t, **sw)) if a.sliding else model.surface
    comps_of = (lambda v: model.components_sliding(v, **sw)) if a.sliding else model.components
    dice, nb = 0.0, 0
    t0 = time.time()
    for s in batch_starts(len(x), a.batch_size, every):
        xb = np.asarray(x[s:s + a.batch_size], dtype=np.float32)
        yb = np.asarray(y[s:s + a.batch_size], dtype=np.float32)
        pb = predict(xb)
        dice += sanity_dice(yb, pb)
        nb += 1
    dt = time.time() - t0
    avg = dice / nb if nb else float("nan")
    print("Average Dice for Test Set = {}".format(avg))
    if a.per_class and nb:
        # (outside the timed loop: the same samples, thresholded at 0.5)
        from .ops import seg_metrics
        K = model.spec.n_cl_out
        stats = [stats_of(np.asarray(x[s:s + a.batch_size], dtype=np.float32),
                          np.asarray(y[s:s + a.batch_size], dtype=np.float32))
                 for s in batch_starts(len(x), a.batch_size, every)]
        m = seg_metrics.metrics_from_case_stats(np.concatenate(stats), int(np.prod(y.shape[1:])) // K)
        tails = [""] * K
        if a.components.strip():              # mean components per case before -> after the filter
            info = np.concatenate([comps_of(np.asarray(x[s:s + a.batch_size], dtype=np.float32))
                                   for s in batch_starts(len(x), a.batch_size, every)]).astype(np.float64)
            tails = [", components = {:.2f} -> {:.2f}".format(info[:, k, 0].mean(), info[:, k, 1].mean())
                     for k in range(K)]
        for k in range(K):
            print("class {}: case Dice = {}, sensitivity = {}, specificity = {}{}".format(
                k, seg_metrics.fmt(m["case_dice"][k]), seg_metrics.fmt(m["sensitivity"][k]),
                seg_metrics.fmt(m["specificity"][k]), tails[k]))
        print("Case Dice = {} ({} cases)".format(seg_metrics.fmt(m["case_dice_mean"]), m["cases"]))
    if a.hd95 and nb:
        from .ops import seg_metrics
        surf = [surface_of(np.asarray(x[s:s + a.batch_size], dtype=np.float32),
                           np.asarray(y[s:s + a.batch_size], dtype=np.float32))
                for s in batch_starts(len(x), a.batch_size, every)]
        m = seg_metrics.hd95_metrics(seg_metrics.accumulate_hd95(np.concatenate(surf), tuple(y.shape[1:-1])))
        for k in range(len(m["hd95"])):
            print("class {}: HD95 = {}".format(k, seg_metrics.fmt(m["hd95"][k])))
        print("HD95 = {} ({} cases)".format(seg_metrics.fmt(m["hd95_mean"]), sum(len(s) for s in surf)))
    print("({} batches, {} backend, {:.1f} images/sec)".format(nb, model.name, nb * a.batch_size / max(dt, 1e-9)))
    return avg


if __name__ == "__main__":
    main()
    sys.exit(0)

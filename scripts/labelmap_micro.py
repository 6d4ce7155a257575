"""Per-launch time of the label-map op (csrc/kernels/labelmap.h) next to its torch definition
(`ops.labelmap.labelmap_torch`) on the device on the same tensors, and what it buys a case:
`Predictor.segment` (labels made on the device, uint8 copied out) against `predict_sliding`
followed by `labelmap_torch` on the host (fp32 probabilities copied out), per case
(profiles/r17_labelmap.md).  Shapes: one case of 155 x 240 x 240 with K = 1 and K = 3, and
1024 slices of 128 x 128 pasted into 240 x 240 at (56, 56).
Every figure is the median of REPS repetitions after a warm-up, with the minimum and the maximum.
`op_us` is the time per call between device events, launch path included; for the kernel's own
time run `--profile case` / `--profile slices` (the op alone, 50 launches per K) under
rocprofv3 --kernel-trace --stats, a run of its own.
Usage on the GPU box: python scripts/labelmap_micro.py [--no-case | --profile case|slices]
(one JSON line per measurement)"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.config import Config  # noqa: E402
from unet_distributed_amd.models import reference  # noqa: E402
from unet_distributed_amd.models.spec import spec_from_config  # noqa: E402
from unet_distributed_amd.ops import labelmap as lm  # noqa: E402
from unet_distributed_amd.runtime.executor_base import sliding_labels  # noqa: E402
from unet_distributed_amd.runtime.params import FlatParams  # noqa: E402

dev = torch.device("cuda:0")
REPS = 7


def spread(fn, iters):
    """{median, min, max} us per call of fn over REPS timed groups of `iters` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return dict(median=statistics.median(out), min=min(out), max=max(out))


def wall(fn):
    """{median, min, max} seconds of fn (host wall clock, device drained) over REPS calls."""
    fn()
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return dict(median=statistics.median(out), min=min(out), max=max(out))


SHAPES = (("case 155x240x240", (1, 155, 240, 240), None, (0, 0, 0)),
          ("1024 slices 128x128 -> 240x240", (1024, 1, 128, 128), (1, 240, 240), (0, 56, 56)))


def op_shapes(only=None):
    C = native.require()
    for name, src, dst, off, K in [s + (K,) for s in SHAPES for K in (1, 3)]:
        if only is not None and not name.startswith(only):
            continue
        g = torch.Generator(device=dev).manual_seed(3)
        prob = torch.rand(src + (K,), generator=g, device=dev)
        rule, values = lm.parse_labels("", K, 5)
        d = src[1:] if dst is None else dst
        moved = prob.numel() * 4 + src[0] * d[0] * d[1] * d[2]               # bytes read + written
        if only is not None:                                                 # (the profiled run: the op alone)
            for _ in range(50):
                sliding_labels(C, prob, 0.5, rule, values, dst, off)
            torch.cuda.synchronize()
            print(json.dumps(dict(what="profile", shape=name, K=K, bytes=moved, launches=50)), flush=True)
            continue
        op = spread(lambda: sliding_labels(C, prob, 0.5, rule, values, dst, off), 500)
        ref = spread(lambda: lm.labelmap_torch(prob, 0.5, rule, values, dst, off), 5)
        a, ac = sliding_labels(C, prob, 0.5, rule, values, dst, off)
        b, bc = lm.labelmap_torch(prob, 0.5, rule, values, dst, off)
        print(json.dumps(dict(what="op", shape=name, K=K, bytes=moved, op_us=op, torch_us=ref,
                              op_GBps=moved / op["median"] / 1e3, torch_GBps=moved / ref["median"] / 1e3,
                              torch_over_op=ref["median"] / op["median"],
                              matches_oracle=bool(torch.equal(a, b) and torch.equal(ac.long(), bc)))), flush=True)
        yield name, K, op["median"]


def case(K, op_us):
    """One case of 155 slices of 240 x 240 through a 2D model of input size 128."""
    from unet_distributed_amd.inference import load_saved_model
    from unet_distributed_amd.utils.checkpoint import export_model
    with tempfile.TemporaryDirectory() as tmp:
        cfg = Config(img_size=128, in_channels=4, out_channels=K, checkpoint_dir=tmp)
        spec = spec_from_config(cfg)
        flat = FlatParams(spec)
        flat.load_dict(reference.init_params(spec, seed=3))
        model = load_saved_model(export_model(cfg, spec, flat), device=dev, batch=128)
    x = np.random.RandomState(1).randn(155, 240, 240, 4).astype(np.float32)
    rule, values = lm.parse_labels("", K, 5)

    def on_host():
        p = torch.from_numpy(model.predict_sliding(x))
        return lm.labelmap_torch(p.unsqueeze(0), 0.5, rule, values)

    seg = wall(lambda: model.segment(x, volume=True, mode=5))
    host = wall(on_host)
    fwd = wall(lambda: model.backend.predict_sliding(torch.from_numpy(x).to(dev), post=False))
    a, ac = model.segment(x, volume=True, mode=5)
    b, bc = on_host()
    print(json.dumps(dict(what="case", K=K, backend=model.name, segment_s=seg, predict_then_host_labelmap_s=host,
                          predict_sliding_device_s=fwd, host_over_segment=host["median"] / seg["median"],
                          op_share_of_segment=op_us * 1e-6 / seg["median"],
                          same_labels=bool(np.array_equal(a, b[0].numpy()) and np.array_equal(ac, bc.numpy())))),
          flush=True)


if __name__ == "__main__":
    if "--profile" in sys.argv:
        list(op_shapes({"case": "case", "slices": "1024"}[sys.argv[sys.argv.index("--profile") + 1]]))
        sys.exit(0)
    ops = {(n, K): us for n, K, us in op_shapes()}
    if "--no-case" not in sys.argv:
        for K in (1, 3):
            case(K, ops[("case 155x240x240", K)])

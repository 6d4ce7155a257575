"""Per-call time of the connected-component filter (csrc/kernels/components.h) through the
executor's `components` at the evaluation shapes -- 2D b1024 128x128 with K = 1 and 3, 3D b8
128^3 with K = 1, bf16 -- next to the executor's evaluation forward and its `case_surface`
(the HD95 op) of the same batch, measured in the same run (profiles/r14_components.md).
The masks are `synthetic_brats` lesions plus specks: every sample gets SPECKS stray blobs of
1 to 8 voxels at random places, the situation the filter exists for.  For the split over the
op's six kernels run it under rocprofv3 --kernel-trace --stats.
Usage on the GPU box: python scripts/components_micro.py   (one JSON line per shape)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd.config import Config  # noqa: E402
from unet_distributed_amd.data.datasets import synthetic_brats  # noqa: E402
from unet_distributed_amd.models import reference  # noqa: E402
from unet_distributed_amd.models.spec import spec_from_config  # noqa: E402
from unet_distributed_amd.ops.components import components_torch  # noqa: E402
from unet_distributed_amd.runtime.backends import NativeBackend  # noqa: E402
from unet_distributed_amd.runtime.params import FlatParams  # noqa: E402

dev = torch.device("cuda:0")
UNIQUE = 64          # distinct synthetic samples, tiled to the batch
SPECKS = 6
POLICIES = (("largest", True, 0), ("min:20", False, 20), ("largest,min:20", True, 20))


def timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def specks(y, rng):
    """The targets plus SPECKS stray blobs of 1..8 voxels (a run along W) per (sample, class)."""
    p = y.copy()
    W = p.shape[-2]
    for n in range(p.shape[0]):
        for k in range(p.shape[-1]):
            for _ in range(SPECKS):
                at = tuple(rng.randint(0, v) for v in p.shape[1:-2])
                x0 = rng.randint(0, W)
                p[(n,) + at + (slice(x0, min(W, x0 + rng.randint(1, 9))), k)] = 1.0
    return p


for B, img, dims, K in ((1024, 128, 2, 1), (1024, 128, 2, 3), (8, 128, 3, 1)):
    cfg = Config(batch_size=B, img_size=img, dims=dims, in_channels=4, out_channels=K, eval_hd95=True,
                 eval_components="largest")
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    nb = NativeBackend(spec, flat, cfg, dev, B)
    e = nb.engine
    e.repack()
    u = min(B, UNIQUE)
    x, y = synthetic_brats(u, img, 4, dims, seed=7, out_channels=K)
    pred = specks(y, np.random.RandomState(11))
    reps = (B // u,) + (1,) * (x.ndim - 1)
    x, y, pred = (torch.from_numpy(np.tile(a, reps)).to(dev) for a in (x, y, pred))
    e.load_batch(x, y)
    fwd = [timeit(e.evaluate_batch, 5) for _ in range(2)]
    # the prediction: lesions and specks at probability 0.9, the rest at 0.1
    e.prob.view(-1).copy_((pred * 0.8 + 0.1).reshape(-1))
    rec = dict(B=B, K=K)
    for name, largest, v in POLICIES:
        rec["op_us[%s]" % name] = min(timeit(lambda: e.components(0.5, largest, v), 5) for _ in range(2))
    surf = [timeit(lambda: e.case_surface(0.5), 5) for _ in range(2)]
    surf_pp = [timeit(lambda: e.case_surface(0.5, post=True), 5) for _ in range(2)]
    info = e.components(0.5, True, 20).cpu()
    check = 2 if dims == 2 else 1
    want_out, want_info = components_torch((pred[:check] * 0.8 + 0.1).cpu(), 0.5, True, 20)
    ok = bool(torch.equal(info[:check], want_info) and torch.equal(e.probs_pp()[:check].cpu(), want_out))
    d, h, w = e.sdims(1)
    op = min(rec["op_us[%s]" % p[0]] for p in POLICIES)
    rec.update(D=d, H=h, W=w, groups=-(-B // e._components_group), scratch_bytes=e.components_scratch.numel() * 4,
               matches_oracle=ok, mean_components=float(info[..., 0].double().mean()),
               mean_kept=float(info[..., 1].double().mean()), eval_forward_us=min(fwd), surf_dist_us=min(surf),
               surf_dist_filtered_us=min(surf_pp), op_over_forward=op / min(fwd), op_over_surf_dist=op / min(surf),
               bytes_min=B * d * h * w * K * 4 * 2, op_GBps_of_min=B * d * h * w * K * 8 / op / 1e3)
    print(json.dumps(rec), flush=True)
    del nb, e, x, y, pred, flat
    torch.cuda.empty_cache()

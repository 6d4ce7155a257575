"""Per-call time of the HD95 surface-distance op (surf_dist.h) through the executor's
`case_surface` at the bench shapes -- 2D b1024 128x128 with K = 1 and 3, 3D b8 128^3 with
K = 1, bf16 -- next to the executor's evaluation forward of the same batch.  The masks are
`synthetic_brats` targets; the prediction is the target shifted by a few voxels (the op's
cost depends on the masks only through the selection's sample count).
Usage on the GPU box: python scripts/surf_dist_micro.py   (one JSON line per shape)"""
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
from unet_distributed_amd.ops.seg_metrics import case_surface_torch  # noqa: E402
from unet_distributed_amd.runtime.backends import NativeBackend  # noqa: E402
from unet_distributed_amd.runtime.params import FlatParams  # noqa: E402

dev = torch.device("cuda:0")
SHIFT = 3
UNIQUE = 64          # distinct synthetic samples, tiled to the batch


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


for B, img, dims, K in ((1024, 128, 2, 1), (1024, 128, 2, 3), (8, 128, 3, 1)):
    cfg = Config(batch_size=B, img_size=img, dims=dims, in_channels=4, out_channels=K, eval_hd95=True)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    nb = NativeBackend(spec, flat, cfg, dev, B)
    e = nb.engine
    e.repack()
    u = min(B, UNIQUE)
    x, y = synthetic_brats(u, img, 4, dims, seed=7, out_channels=K)
    reps = (B // u,) + (1,) * (x.ndim - 1)
    x, y = torch.from_numpy(np.tile(x, reps)).to(dev), torch.from_numpy(np.tile(y, reps)).to(dev)
    e.load_batch(x, y)
    fwd = [timeit(e.evaluate_batch, 5) for _ in range(2)]
    # the prediction: the target shifted by SHIFT voxels along W (probabilities 0.9 / 0.1)
    pred = torch.zeros_like(y)
    pred[..., SHIFT:, :] = y[..., :-SHIFT, :]
    e.prob.view(-1).copy_((pred * 0.8 + 0.1).reshape(-1))
    op = [timeit(lambda: e.case_surface(0.5), 5) for _ in range(2)]
    surf = e.case_surface(0.5).cpu().long()
    check = 2 if dims == 2 else 1
    ok = bool(torch.equal(surf[:check], case_surface_torch((pred[:check] * 0.8 + 0.1).cpu(), y[:check].cpu(), 0.5)))
    d, h, w = e.sdims(1)
    groups = -(-B // e._case_surface_group)
    rec = dict(B=B, D=d, H=h, W=w, K=K, groups=groups, scratch_bytes=e.case_surface_scratch.numel() * 4,
               matches_oracle=ok, mean_surface_voxels=float(surf[..., :2].double().mean()),
               op_us_0=op[0], op_us_1=op[1], eval_forward_us_0=fwd[0], eval_forward_us_1=fwd[1],
               op_over_forward=min(op) / min(fwd))
    print(json.dumps(rec), flush=True)
    del nb, e, x, y, pred, flat
    torch.cuda.empty_cache()

"""Per-launch time of the sliding-window ops (csrc/kernels/sliding.h) next to the evaluation
forward of the same batch of tiles, and end-to-end images/s of `predict_sliding`
(profiles/r13_sliding.md).  Workloads: 2D 240 x 240 x 4 slices at tile 128, overlap 0.5, B = 1024,
K = 1 and 3 (9 tiles per slice); 3D 155 x 240 x 240 x 4 volumes at tile 128^3, B = 8 (18 tiles per
volume).  Device-event time of back-to-back launches on a full batch (t0 = 0, nt = B), cases
interleaved and repeated; bytes are what the shapes require (extract: the batch read and written;
blend: the batch's probabilities and weights read, the touched images' accumulator read and
written; finish: the accumulator read and written, the summed weights read).

Usage on the GPU box: python scripts/sliding_micro.py            (one JSON line per workload)
                      python scripts/sliding_micro.py --once     (two `predict_sliding` calls per
                      workload and nothing else: the run to put under rocprofv3 --kernel-trace --stats)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.ops import sliding  # noqa: E402

C = native.require()
dev = torch.device("cuda:0")
REPS = 3
HBM_PEAK = 8.0e12       # bytes/s


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters      # us


def workload(dims, B, K, N, img, once):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(batch_size=B, dims=dims, img_size=128, in_channels=4, out_channels=K, hip_graph=False)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    nb = NativeBackend(spec, flat, cfg, dev, B)
    e = nb.engine
    e.repack()
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn((N,) + img + (4,), device=dev, generator=g)
    T = sliding.tile_shape(128, dims)
    stride = sliding.strides(T, 0.5)
    d3 = img if dims == 3 else (1,) + img
    tpi = sliding.tiles_per_image(d3, T, stride)
    total = N * tpi
    rec = dict(dims=dims, image=list(img), N=N, B=B, K=K, tiles_per_image=tpi, tiles=total,
               batches=-(-total // B))
    if once:
        for _ in range(2):
            nb.predict_sliding(x, 0.5, "gaussian")
        torch.cuda.synchronize()
        print(json.dumps(rec), flush=True)
        return
    e.plan_sliding()
    acc =torch.zeros((N,) + d3 + (K,), device=dev)
    wsum = sliding.weight_sum(d3, T, stride, "gaussian").to(dev)
    st = int(torch.cuda.current_stream().cuda_stream)
    head, tail = [N] + list(d3), list(T) + list(stride) + [B, 0, B]
    tile_px = T[0] * T[1] * T[2]
    imgs = (B - 1) // tpi + 1
    P = d3[0] * d3[1] * d3[2]
    nbytes = {"sw_extract": 2 * B * tile_px * 4 * 4,
              "sw_blend": B * tile_px * K * 4 + tile_px * 4 + 2 * imgs * P * K * 4,
              "sw_finish": 2 * N * P * K * 4 + P * 4}
    cases = {
        "sw_extract": lambda: C.generic("sw_extract", [x.data_ptr(), e.sw_x.data_ptr()], head + [4] + tail, [], st, 0),
        "load+forward": lambda: (e.load_batch(e.sw_x, e.sw_y), e.evaluate_batch()),
        "sw_blend": lambda: C.generic("sw_blend", [e.prob.data_ptr(), e.sw_w[1].data_ptr(), acc.data_ptr()],
                                      head + [K] + tail, [], st, 0),
        "sw_finish": lambda: (acc.fill_(1.0), C.generic("sw_finish", [acc.data_ptr(), wsum.data_ptr()], head + [K], [],
                                                        st, 0)),
        "fill": lambda: acc.fill_(1.0),
        "predict_sliding": lambda: nb.predict_sliding(x, 0.5, "gaussian"),
    }
    iters = {"load+forward": 5, "predict_sliding": 2}
    rec["us"] = {}
    for rep in range(REPS):
        for name, fn in cases.items():              # interleaved: every case once per repetition
            rec["us"].setdefault(name, []).append(round(timed(fn, iters.get(name, 20)), 1))
    med = {c: float(np.median(v)) for c, v in rec["us"].items()}
    med["sw_finish"] = med["sw_finish"] - med["fill"]           # (the refill keeps the quotient finite)
    rec["median_us"] = med
    rec["bytes"] = nbytes
    rec["TBps"] = {c: round(nbytes[c] / med[c] / 1e6, 3) for c in nbytes}
    rec["of_hbm_peak"] = {c: round(nbytes[c] / med[c] * 1e6 / HBM_PEAK, 3) for c in nbytes}
    per_batch = med["sw_extract"] + med["sw_blend"] + med["sw_finish"] / rec["batches"]
    rec["ops_per_batch_over_forward"] = round(per_batch / med["load+forward"], 4)
    rec["images_per_s"] = round(N / med["predict_sliding"] * 1e6, 2)
    rec["tiles_per_s"] = round(total / med["predict_sliding"] * 1e6, 1)
    print(json.dumps(rec), flush=True)


once = "--once" in sys.argv[1:]
for dims, B, K, N, img in ((2, 1024, 1, 512, (240, 240)), (2, 1024, 3, 512, (240, 240)), (3, 8, 1, 2, (155, 240, 240))):
    torch.cuda.empty_cache()
    workload(dims, B, K, N, img, once)

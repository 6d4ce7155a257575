"""Per-launch time of the test-time augmentation ops (csrc/kernels/tta.h) next to
`torch.add(acc, prob, out=acc)` on the same tensors in the same process -- the same three
streams as tta_acc in add mode -- cases interleaved and repeated (profiles/r12_tta.md).
Shapes: b1024 128x128 K = 1 and K = 3, b8 128^3 K = 1.  The launches rotate over four
(prob, acc) pairs so no pass re-reads the 256 MiB Infinity Cache.

`--engine` adds, per shape, the executor's evaluation forward, the augmenting gather and one
whole `evaluate_tta` at `flip` and `flip,rot90` (device events around the calls).
Usage on the GPU box: python scripts/tta_micro.py [--engine]   (one JSON line per shape)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.data.augment import apply_torch, tta_codes  # noqa: E402

C = native.require()
dev = torch.device("cuda:0")
ITERS, REPS, SETS = 100, 3, 4


def timed(fn, iters):
    for i in range(SETS):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters      # us


def ops(N, D, H, K):
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (N, H, H, K) if D == 1 else (N, D, H, H, K)
    probs = [torch.rand(shape, device=dev, generator=g) for _ in range(SETS)]
    accs = [torch.rand(shape, device=dev, generator=g) for _ in range(SETS)]
    # (the finish's own pairs: prob = (acc + prob) / 2 stays in [0, 1] however often it runs)
    fprobs = [torch.rand(shape, device=dev, generator=g) for _ in range(SETS)]
    faccs = [torch.rand(shape, device=dev, generator=g) for _ in range(SETS)]
    tgt = (torch.rand(shape, device=dev, generator=g) > 0.6).to(torch.bfloat16)
    total = probs[0].numel()
    part = torch.zeros(C.tta_finish_blocks(total) * 4, device=dev)
    sums = torch.zeros(4, device=dev)
    st = int(torch.cuda.current_stream().cuda_stream)
    flip, swap = (3 if D == 1 else 11), 5

    def acc_op(code, mode):
        return lambda i: C.generic("tta_acc", [probs[i % SETS].data_ptr(), accs[i % SETS].data_ptr()],
                                   [N, D, H, H, K, code, mode], [], st, 0)
    cases = {"torch_add": lambda i: torch.add(accs[i % SETS], probs[i % SETS], out=accs[i % SETS]),
             "acc_identity": acc_op(0, 1), "acc_flip": acc_op(flip, 1), "acc_swap": acc_op(swap, 1),
             "acc_swap_flip": acc_op(swap | 2, 1), "acc_identity_write": acc_op(0, 0),
             "finish": lambda i: C.generic("tta_finish", [fprobs[i % SETS].data_ptr(), faccs[i % SETS].data_ptr(),
                                                          tgt.data_ptr(), part.data_ptr(), sums.data_ptr()],
                                           [total], [0.5], st, 0)}
    # results first: write mode of the swap code is apply_torch's permutation
    acc_op(swap | 2, 0)(0)
    torch.cuda.synchronize()
    ok = bool(torch.equal(accs[0], apply_torch(probs[0], probs[0], [swap | 2] * N)[0]))
    rec = dict(N=N, D=D, H=H, K=K, bytes_3_streams=3 * total * 4, iters=ITERS, matches_apply_torch=ok, us={})
    for rep in range(REPS):
        for name, fn in cases.items():              # interleaved: every case once per repetition
            rec["us"].setdefault(name, []).append(round(timed(fn, ITERS), 2))
    add = rec["us"]["torch_add"]
    rec["torch_add_spread"] = round(max(add) / min(add) - 1.0, 4)
    rec["ratio_to_torch_add"] = {c: round(float(np.median(v) / np.median(add)), 4) for c, v in rec["us"].items()}
    rec["TBps"] = {c: round((2 if c.endswith("write") else 3) * total * 4 / float(np.median(v)) / 1e6, 3)
                   for c, v in rec["us"].items() if c != "finish"}
    print(json.dumps(rec), flush=True)


def engine(B, dims, H, K):
    from unet_distributed_amd.config import Config
    from unet_distributed_amd.models import reference
    from unet_distributed_amd.models.spec import spec_from_config
    from unet_distributed_amd.runtime.backends import NativeBackend
    from unet_distributed_amd.runtime.params import FlatParams
    cfg = Config(batch_size=B, dims=dims, img_size=H, in_channels=4, out_channels=K, eval_tta="flip,rot90",
                 hip_graph=False)
    spec = spec_from_config(cfg)
    flat = FlatParams(spec, device=dev)
    flat.load_dict(reference.init_params(spec, seed=3))
    nb = NativeBackend(spec, flat, cfg, dev, B)
    e = nb.engine
    e.repack()
    g = torch.Generator(device=dev).manual_seed(2)
    sp = (H,) * dims
    x = torch.randn((B,) + sp + (4,), device=dev, generator=g)
    y = (torch.rand((B,) + sp + (K,), device=dev, generator=g) > 0.6).float()
    iota = torch.arange(B, device=dev)
    code = torch.full((B,), 5, dtype=torch.int32, device=dev)
    iters = 10
    rec = dict(B=B, dims=dims, H=H, K=K, iters=iters, us={})
    cases = {"eval_forward": lambda i: e.evaluate_batch(),
             "gather_aug": lambda i: e.load_indexed(x, y, iota, aug=(code, None))}
    for spec_name in ("flip", "flip,rot90"):
        codes = tta_codes(spec_name, dims)
        cases["evaluate_tta:%s:M%d" % (spec_name, len(codes))] = lambda i, c=codes: e.evaluate_tta(x, y, c)
    for rep in range(REPS):
        for name, fn in cases.items():
            rec["us"].setdefault(name, []).append(round(timed(fn, iters), 1))
    rec["median_us"] = {c: float(np.median(v)) for c, v in rec["us"].items()}
    print(json.dumps(rec), flush=True)


SHAPES = [(1024, 1, 128, 1), (1024, 1, 128, 3), (8, 128, 128, 1)]
for N, D, H, K in SHAPES:
    torch.cuda.empty_cache()
    ops(N, D, H, K)
if "--engine" in sys.argv[1:]:
    for N, D, H, K in SHAPES:
        torch.cuda.empty_cache()
        engine(N, 2 if D == 1 else 3, H, K)

"""Per-launch time of the evaluation-statistics kernel (seg_stats.h) at the bench shapes --
2D b1024 128x128 with K = 1 and 3, 3D b8 128^3 with K = 1, bf16 target -- against the same
statistics from torch ops on the same buffers.  Inputs rotate over more than twice the
256 MiB Infinity Cache ("rotating": the HBM figure); "same_buffer" re-reads one pair.
Usage on the GPU box: python scripts/seg_stats_micro.py   (one JSON line per shape)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402

C = native.require()
dev = torch.device("cuda:0")


def torch_stats(prob, tgt, N, S, K, thr):
    p = prob.view(N, S, K)
    t = tgt.view(N, S, K).float()
    pos, fg = p >= thr, t >= 0.5
    return torch.stack([(t * p).sum(1), t.sum(1), p.sum(1), (pos & fg).sum(1).float(), (pos & ~fg).sum(1).float(),
                        (~pos & fg).sum(1).float()], dim=-1)


def timeit(fn, iters):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


for N, S, K in ((1024, 128 * 128, 1), (1024, 128 * 128, 3), (8, 128 ** 3, 1)):
    nbytes = N * S * K * 6
    copies = max(2, -(-(640 << 20) // nbytes))            # rotate over > 2x the 256 MiB Infinity Cache
    g = torch.Generator(device=dev).manual_seed(1)
    probs = [torch.rand(N * S * K, device=dev, generator=g) for _ in range(copies)]
    tgts = [(torch.rand(N * S * K, device=dev, generator=g) > 0.6).to(torch.bfloat16) for _ in range(copies)]
    stats = torch.zeros(N, K, 6, device=dev)
    chunks = C.seg_stats_chunks(N, S, K)
    part = torch.zeros(N * chunks * 6 * K, device=dev)
    st = int(torch.cuda.current_stream().cuda_stream)

    def kern(i, rot=True):
        j = i % copies if rot else 0
        C.generic("seg_stats", [probs[j].data_ptr(), tgts[j].data_ptr(), stats.data_ptr(), part.data_ptr()],
                  [N, S, K], [0.5], st, 0)

    def ref(i, rot=True):
        j = i % copies if rot else 0
        return torch_stats(probs[j], tgts[j], N, S, K, 0.5)

    kern(0)
    want = ref(0)
    torch.cuda.synchronize()
    ok = bool(torch.equal(stats[..., 3:], want[..., 3:]) and torch.allclose(stats[..., :3], want[..., :3], rtol=1e-3))
    rec = dict(N=N, S=S, K=K, chunks=chunks, bytes=nbytes, copies=copies, matches_torch=ok)
    for rep in range(2):
        rec["kernel_us_rotating_%d" % rep] = timeit(kern, 200)
        rec["torch_us_rotating_%d" % rep] = timeit(ref, 20)
        rec["kernel_us_same_buffer_%d" % rep] = timeit(lambda i: kern(i, False), 200)
    rec["kernel_TBps_rotating"] = nbytes / min(rec["kernel_us_rotating_0"], rec["kernel_us_rotating_1"]) / 1e6
    print(json.dumps(rec), flush=True)
    del probs, tgts
    torch.cuda.empty_cache()

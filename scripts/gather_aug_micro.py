"""Per-launch time of the augmenting batch gather (gather.h) at the bench shape -- batch
1024 of 128x128x4, one target channel, bf16 -- next to the plain gather_batch kernel on the
same buffers in the same process, cases interleaved and repeated (profiles/r9_augment.md).
The batch is drawn (sorted indices, as the feeder sends them) from a resident set four
times the batch (5.4 GB) and the outputs rotate over four buffer pairs, so no pass re-reads
the 256 MiB Infinity Cache.  The pass moves 268 + 67 MB in and 134 + 34 MB out.

`--sweep` adds the same pixel count as 64x64 and 32x32 images (one 32-pixel tile row is then
half a row / a whole row of the image: the tile kernel's global segments grow to those of
the plain kernel while its workgroup structure stays).
Usage on the GPU box: python scripts/gather_aug_micro.py [--sweep]   (one JSON line per shape)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.data.augment import apply_torch  # noqa: E402

C = native.require()
dev = torch.device("cuda:0")
CIN, CPAD, K = 4, 4, 1
ITERS, REPS, SETS = 300, 3, 4


def run(B, H, names):
    NALL, P = 4 * B, H * H
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(2)
    x_all = torch.randn(NALL, H, H, CIN, device=dev, generator=g)
    y_all = (torch.rand(NALL, H, H, K, device=dev, generator=g) > 0.6).float()
    idxs = [torch.from_numpy(np.sort(rng.choice(NALL, B, replace=False))).to(dev) for _ in range(SETS)]
    outs = [(torch.empty(B, H, H, CPAD, dtype=torch.bfloat16, device=dev),
             torch.empty(B, H, H, K, dtype=torch.bfloat16, device=dev)) for _ in range(SETS)]
    st = int(torch.cuda.current_stream().cuda_stream)

    def codes(lo, hi):
        return torch.from_numpy(rng.integers(lo, hi, B).astype(np.int32)).to(dev)

    a = 0.1
    affine = torch.stack([1 - a + 2 * a * torch.rand(B, CIN, device=dev, generator=g),
                          -a + 2 * a * torch.rand(B, CIN, device=dev, generator=g)], dim=-1).contiguous()
    mixed = codes(0, 8)
    cases = {"plain": None, "identity": (torch.zeros(B, dtype=torch.int32, device=dev), None),
             "flips": (codes(0, 4), None), "all_T": (codes(4, 8), None), "mixed": (mixed, None),
             "mixed_intensity": (mixed, affine)}
    cases = {k: cases[k] for k in names}

    def launch(case, i):
        j = i % SETS
        xb, tb = outs[j]
        if cases[case] is None:
            C.generic("gather_batch", [x_all.data_ptr(), y_all.data_ptr(), idxs[j].data_ptr(), xb.data_ptr(),
                                       tb.data_ptr()], [B, P, CIN, CPAD, K], [], st, 0)
            return
        code, aff = cases[case]
        C.generic("gather_batch_aug", [x_all.data_ptr(), y_all.data_ptr(), idxs[j].data_ptr(), code.data_ptr(),
                                       aff.data_ptr() if aff is not None else 0, xb.data_ptr(), tb.data_ptr()],
                  [B, 1, H, H, CIN, CPAD, K], [], st, 0)

    def timeit(case):
        for i in range(SETS):
            launch(case, i)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(ITERS):
            launch(case, i)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / ITERS      # us

    # results first: the last case's batch is the permutation of the plain batch that apply_torch gives
    last = names[-1] if cases[names[-1]] is not None and cases[names[-1]][1] is None else "all_T"
    launch("plain", 0)
    torch.cuda.synchronize()
    px, pt = outs[0][0].clone(), outs[0][1].clone()
    launch(last, 0)
    torch.cuda.synchronize()
    wx, wt = apply_torch(px, pt, cases[last][0])
    ok = bool(torch.equal(outs[0][0].view(torch.int16), wx.view(torch.int16))
              and torch.equal(outs[0][1].view(torch.int16), wt.view(torch.int16)))
    del px, pt, wx, wt

    nbytes = B * P * (CIN * 4 + K * 4 + CPAD * 2 + K * 2)
    rec = dict(B=B, H=H, Cin=CIN, Cpad=CPAD, K=K, bytes=nbytes, iters=ITERS, checked=last, matches_apply_torch=ok,
               us={})
    for rep in range(REPS):
        for case in cases:                          # interleaved: every case once per repetition
            rec["us"].setdefault(case, []).append(round(timeit(case), 2))
    plain = rec["us"]["plain"]
    rec["plain_spread"] = round(max(plain) / min(plain) - 1.0, 4)
    rec["ratio_to_plain"] = {c: round(float(np.median(v) / np.median(plain)), 4) for c, v in rec["us"].items()}
    rec["TBps"] = {c: round(nbytes / float(np.median(v)) / 1e6, 3) for c, v in rec["us"].items()}
    print(json.dumps(rec), flush=True)


run(1024, 128, ["plain", "identity", "flips", "all_T", "mixed_intensity", "mixed"])
if "--sweep" in sys.argv[1:]:
    for B, H in ((4096, 64), (16384, 32)):
        torch.cuda.empty_cache()
        run(B, H, ["plain", "identity", "all_T"])

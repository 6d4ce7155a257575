"""Per-launch time of the cropping batch gather (gather.h) at the bench shape -- batch
1024 of 128x128x4 patches, one target channel, bf16 -- next to the augmenting gather
(gather.h, the yardstick) on a 128x128 resident set in the same process, cases
interleaved and repeated (profiles/r15_crop.md).  The 128x128 set is four times the batch
(1.3 GB), the 240x240 set twice the batch (2.4 GB); the batches are sorted indices, as the
feeder sends them, and the outputs rotate over four buffer pairs, so no pass re-reads the
256 MiB Infinity Cache.  Every pass writes 134 + 34 MB and reads 268 + 67 MB of pixels (the
cropping cases in 2 KiB row segments of 3.75 KiB rows).  The `_aligned` cases are the same
batches with every w origin rounded down to 32 pixels, so that each row segment starts on a
128-byte line: what is left of the cost is the pitch, not the partial lines at segment ends.

`--3d` adds the same pixel count as batch 8 of 128^3 patches out of 155x240x240 volumes.
Usage on the GPU box: python scripts/gather_crop_micro.py [--3d]   (one JSON line per shape)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.data.augment import apply_torch, crop_torch  # noqa: E402

C = native.require()
dev = torch.device("cuda:0")
CIN, CPAD, K = 4, 4, 1
ITERS, REPS, SETS = 300, 3, 4


def run(B, patch, stored, nall_plain, nall_crop, names):
    """patch / stored: (D, H, W); the yardstick set is of the patch's size."""
    D, H, W = patch
    Ds, Hs, Ws = stored
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(2)
    sq = (lambda n, s: (n,) + (tuple(s) if s[0] > 1 or D > 1 else tuple(s[1:])))
    sets = {}
    if nall_plain:
        sets["plain"] = (torch.randn(sq(nall_plain, patch) + (CIN,), device=dev, generator=g),
                         (torch.rand(sq(nall_plain, patch) + (K,), device=dev, generator=g) > 0.6).float())
    sets["crop"] = (torch.randn(sq(nall_crop, stored) + (CIN,), device=dev, generator=g),
                    (torch.rand(sq(nall_crop, stored) + (K,), device=dev, generator=g) > 0.6).float())
    idxs = {k: [torch.from_numpy(np.sort(rng.choice(len(v[0]), B, replace=False))).to(dev) for _ in range(SETS)]
            for k, v in sets.items()}
    outs = [(torch.empty(sq(B, patch) + (CPAD,), dtype=torch.bfloat16, device=dev),
             torch.empty(sq(B, patch) + (K,), dtype=torch.bfloat16, device=dev)) for _ in range(SETS)]
    st = int(torch.cuda.current_stream().cuda_stream)
    ncode = 16 if D > 1 else 8

    def codes(lo, hi):
        return torch.from_numpy(rng.integers(lo, hi, B).astype(np.int32)).to(dev)

    a = 0.1
    affine = torch.stack([1 - a + 2 * a * torch.rand(B, CIN, device=dev, generator=g),
                          -a + 2 * a * torch.rand(B, CIN, device=dev, generator=g)], dim=-1).contiguous()
    origin = torch.from_numpy(np.stack([rng.integers(0, s - t + 1, B) for s, t in zip(stored, patch)],
                                       axis=1).astype(np.int32)).to(dev)
    # the same origins with w rounded down to a multiple of 32 pixels: every row segment of the image
    # (16 bytes a pixel) and of the target (4 bytes a pixel) then starts on a 128-byte line
    aligned = origin.clone()
    aligned[:, 2] = aligned[:, 2] // 32 * 32
    zero, mixed = torch.zeros(B, dtype=torch.int32, device=dev), codes(0, ncode)
    swapped = torch.from_numpy((rng.integers(0, ncode // 8, B) * 8 + rng.integers(4, 8, B)).astype(np.int32)).to(dev)
    # case: (resident set, code, affine, origins)
    cases = {"aug_identity": ("plain", zero, None, None), "aug_all_T": ("plain", swapped, None, None),
             "crop_identity": ("crop", zero, None, origin), "crop_null_code": ("crop", None, None, origin),
             "crop_identity_aligned": ("crop", zero, None, aligned), "crop_all_T": ("crop", swapped, None, origin),
             "crop_all_T_aligned": ("crop", swapped, None, aligned), "crop_mixed": ("crop", mixed, None, origin),
             "crop_mixed_intensity": ("crop", mixed, affine, origin)}
    cases = {k: cases[k] for k in names}

    def launch(case, i):
        j = i % SETS
        xb, tb = outs[j]
        which, code, aff, org = cases[case]
        x_all, y_all = sets[which]
        if which == "plain":
            C.generic("gather_batch_aug", [x_all.data_ptr(), y_all.data_ptr(), idxs[which][j].data_ptr(),
                                           code.data_ptr(), aff.data_ptr() if aff is not None else 0, xb.data_ptr(),
                                           tb.data_ptr()], [B, D, H, W, CIN, CPAD, K], [], st, 0)
            return
        C.generic("gather_batch_crop", [x_all.data_ptr(), y_all.data_ptr(), idxs[which][j].data_ptr(),
                                        org.data_ptr(), code.data_ptr() if code is not None else 0,
                                        aff.data_ptr() if aff is not None else 0, xb.data_ptr(), tb.data_ptr()],
                  [B, Ds, Hs, Ws, D, H, W, CIN, CPAD, K], [], st, 0)

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

    # results first: the first samples of the mixed batch against the definition in torch
    chk = "crop_mixed" if "crop_mixed" in cases else names[-1]
    launch(chk, 0)
    torch.cuda.synchronize()
    n = min(B, 16)
    x_all, y_all = sets["crop"]
    sel = idxs["crop"][0][:n]
    code = cases[chk][1]
    wx, wt = apply_torch(*crop_torch(x_all.index_select(0, sel), y_all.index_select(0, sel), origin[:n], patch),
                         (code if code is not None else zero)[:n])
    ok = bool(torch.equal(outs[0][0][:n].view(torch.int16), wx.to(torch.bfloat16).view(torch.int16))
              and torch.equal(outs[0][1][:n].view(torch.int16), wt.to(torch.bfloat16).view(torch.int16)))
    del wx, wt

    P = D * H * W
    nbytes = B * P * (CIN * 4 + K * 4 + CPAD * 2 + K * 2)
    rec = dict(B=B, patch=list(patch), stored=list(stored), Cin=CIN, Cpad=CPAD, K=K, bytes=nbytes, iters=ITERS,
               resident_GB={k: round((v[0].numel() + v[1].numel()) * 4 / 1e9, 2) for k, v in sets.items()},
               checked=chk, matches_torch=ok, us={})
    for rep in range(REPS):
        for case in cases:                          # interleaved: every case once per repetition
            rec["us"].setdefault(case, []).append(round(timeit(case), 2))
    base = rec["us"][names[0]]
    rec["base"] = names[0]
    rec["base_spread"] = round(max(base) / min(base) - 1.0, 4)
    rec["ratio_to_base"] = {c: round(float(np.median(v) / np.median(base)), 4) for c, v in rec["us"].items()}
    rec["TBps"] = {c: round(nbytes / float(np.median(v)) / 1e6, 3) for c, v in rec["us"].items()}
    print(json.dumps(rec), flush=True)


run(1024, (1, 128, 128), (1, 240, 240), 4096, 2048,
    ["aug_identity", "aug_all_T", "crop_identity", "crop_null_code", "crop_identity_aligned", "crop_all_T",
     "crop_all_T_aligned", "crop_mixed", "crop_mixed_intensity"])
if "--3d" in sys.argv[1:]:
    sets = None
    torch.cuda.empty_cache()
    ITERS = 100
    run(8, (128, 128, 128), (155, 240, 240), 0, 16, ["crop_identity", "crop_mixed", "crop_mixed_intensity"])

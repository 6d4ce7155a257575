"""Per-launch time of the elastic batch gather (gather_resample.h) at the bench shape -- batch 1024
of 128x128x4 patches out of 240x240 slices, bf16 -- next to the resampling gather (gather_resample.h)
and the cropping gather (gather.h, the yardstick) on the same resident set in the same
process, cases interleaved and repeated (profiles/r19_elastic.md).  The 240x240 set is twice the
batch (2.4 GB); the batches are sorted indices, as the feeder sends them, and the outputs rotate
over four buffer pairs, so no pass re-reads the 256 MiB Infinity Cache.  Matrices are
draw_spatial's at the default ranges (30 degrees, a = 0.25), fields draw_elastic's at cell 32
with 4 pixels and at cell 8 with 1 pixel (the largest the flags admit), codes mixed.  Cases: the
crop, the warp, the elastic gather with a zero field (the warp's pixels: what the displacement's
arithmetic and the staging cost on their own), with drawn fields at both cells, without matrices,
and with the intensity affine.

Rows: bf16 K = 1, bf16 K = 3, the fp32 op, and with `--3d` the same pixel count as batch 8 of
128^3 patches out of 155x240x240 volumes.
Usage on the GPU box: python scripts/gather_elastic_micro.py [--3d]   (one JSON line per row)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.data.augment import apply_torch, draw_elastic, draw_spatial, elastic_torch  # noqa: E402

C = native.require()
dev = torch.device("cuda:0")
CIN = 4
ITERS, REPS, SETS = 300, 3, 4


def run(B, patch, stored, nall, K, fp32, names):
    """patch / stored: (D, H, W)."""
    D, H, W = patch
    Ds, Hs, Ws = stored
    dt, pre, cpad = (torch.float32, "f32_", CIN) if fp32 else (torch.bfloat16, "", 4)
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(2)
    sq = (lambda n, s: (n,) + (tuple(s) if D > 1 else tuple(s[1:])))
    x_all = torch.randn(sq(nall, stored) + (CIN,), device=dev, generator=g)
    y_all = (torch.rand(sq(nall, stored) + (K,), device=dev, generator=g) > 0.6).float()
    idxs = [torch.from_numpy(np.sort(rng.choice(nall, B, replace=False))).to(dev) for _ in range(SETS)]
    outs = [(torch.empty(sq(B, patch) + (cpad,), dtype=dt, device=dev),
             torch.empty(sq(B, patch) + (K,), dtype=dt, device=dev)) for _ in range(SETS)]
    st = int(torch.cuda.current_stream().cuda_stream)
    ncode = 16 if D > 1 else 8
    a = 0.1
    affine = torch.stack([1 - a + 2 * a * torch.rand(B, CIN, device=dev, generator=g),
                          -a + 2 * a * torch.rand(B, CIN, device=dev, generator=g)], dim=-1).contiguous()
    origin = torch.from_numpy(np.stack([rng.integers(0, s - t + 1, B) for s, t in zip(stored, patch)],
                                       axis=1).astype(np.int32)).to(dev)
    mixed = torch.from_numpy(rng.integers(0, ncode, B).astype(np.int32)).to(dev)
    drawn = torch.from_numpy(draw_spatial(3, 7, np.arange(B), "rotate,scale", 30.0, 0.25)).to(dev)
    f32 = torch.from_numpy(draw_elastic(3, 7, np.arange(B), H, 4.0, 32)).to(dev)
    f8 = torch.from_numpy(draw_elastic(3, 7, np.arange(B), H, 1.0, 8)).to(dev)
    # case: (affine, matrices, (field, cell) or None for the warp; matrices None too: the crop)
    cases = {"crop_mixed": (None, None, None), "warp_drawn_mixed": (None, drawn, None),
             "elastic_zero_cell32": (None, drawn, (torch.zeros_like(f32), 32)),
             "elastic_cell32": (None, drawn, (f32, 32)), "elastic_cell8": (None, drawn, (f8, 8)),
             "elastic_cell32_no_matrix": (None, None, (f32, 32)),
             "elastic_cell32_intensity": (affine, drawn, (f32, 32))}
    cases = {k: cases[k] for k in names}
    ints = [B, Ds, Hs, Ws, D, H, W, CIN, cpad, K]

    def launch(case, i):
        j = i % SETS
        xb, tb = outs[j]
        aff, mat, fld = cases[case]
        head = [x_all.data_ptr(), y_all.data_ptr(), idxs[j].data_ptr(), origin.data_ptr(), mixed.data_ptr()]
        affp = aff.data_ptr() if aff is not None else 0
        matp = mat.data_ptr() if mat is not None else 0
        tail = [xb.data_ptr(), tb.data_ptr()]
        if fld is not None:
            C.generic(pre + "gather_batch_elastic", head + [matp, affp, fld[0].data_ptr()] + tail,
                      ints + [fld[1].bit_length() - 1], [], st, 0)
        elif mat is None:
            C.generic(pre + "gather_batch_crop", head + [affp] + tail, ints, [], st, 0)
        else:
            C.generic(pre + "gather_batch_warp", head + [matp, affp] + tail, ints, [], st, 0)

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

    # results first: the first samples of the drawn batches against the definition in torch
    bits = torch.int32 if fp32 else torch.int16
    n = min(B, 2 if D > 1 else 16)
    ok = {}
    for chk in [c for c in names if c in ("elastic_cell32", "elastic_cell8")]:
        launch(chk, 0)
        torch.cuda.synchronize()
        sel = idxs[0][:n]
        fld, cell = cases[chk][2]
        wx, wt = apply_torch(*elastic_torch(x_all.index_select(0, sel), y_all.index_select(0, sel), origin[:n], patch,
                                            drawn[:n], fld[:n], cell), mixed[:n])
        ok[chk] = bool(torch.equal(outs[0][0][:n].view(bits), wx.to(dt).view(bits))
                       and torch.equal(outs[0][1][:n].view(bits), wt.to(dt).view(bits)))
        del wx, wt

    P = D * H * W
    eb = 4 if fp32 else 2
    nbytes = B * P * (CIN * 4 + K * 4 + cpad * eb + K * eb)       # (of the crop: the others read four taps)
    rec = dict(B=B, patch=list(patch), stored=list(stored), Cin=CIN, Cpad=cpad, K=K, out="fp32" if fp32 else "bf16",
               bytes=nbytes, iters=ITERS, resident_GB=round((x_all.numel() + y_all.numel()) * 4 / 1e9, 2),
               matches_torch=ok, us={})
    for rep in range(REPS):
        for case in cases:                          # interleaved: every case once per repetition
            rec["us"].setdefault(case, []).append(round(timeit(case), 2))
    for base in names[:2]:
        b = rec["us"][base]
        rec["spread_" + base] = round(max(b) / min(b) - 1.0, 4)
        rec["ratio_to_" + base] = {c: round(float(np.median(v) / np.median(b)), 4) for c, v in rec["us"].items()}
    print(json.dumps(rec), flush=True)


ALL = ["crop_mixed", "warp_drawn_mixed", "elastic_zero_cell32", "elastic_cell32", "elastic_cell8",
       "elastic_cell32_no_matrix", "elastic_cell32_intensity"]
run(1024, (1, 128, 128), (1, 240, 240), 2048, 1, False, ALL)
torch.cuda.empty_cache()
run(1024, (1, 128, 128), (1, 240, 240), 2048, 3, False, ALL[:5])
torch.cuda.empty_cache()
run(1024, (1, 128, 128), (1, 240, 240), 2048, 1, True, ALL[:5])
if "--3d" in sys.argv[1:]:
    torch.cuda.empty_cache()
    ITERS = 100
    run(8, (128, 128, 128), (155, 240, 240), 16, 1, False, ALL[:5])

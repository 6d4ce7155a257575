"""Per-launch time of the 3D resampling batch gather (gather_batch_warp3, gather_resample.h) at the 3D
bench shape -- batch 8 of 128^3 x 4 patches out of 155 x 240 x 240 x 4 volumes -- next to the in-plane
gather_batch_warp and gather_batch_elastic (the yardsticks) on the same resident set in the same
process, cases interleaved and repeated (profiles/r21_rotate3d.md).  The set is twice the batch
(2.3 GB + targets); the batches are sorted indices, as the feeder sends them, and the outputs
rotate over four buffer pairs.  Matrices: the identity, draw_spatial3's at the defaults (30 / 15
degrees, a = 0.25), 30 degrees about each single axis; fields draw_elastic's at cell 32 with 4
pixels.  Before timing, the first two volumes of the drawn batches are compared with the
definition in torch.

Rows: bf16 K = 1, and without `--quick` bf16 K = 3 and the fp32 op.
Usage on the GPU box: python scripts/gather_warp3_micro.py [--quick] [--lib PATH]   (one JSON line per row;
--lib: an extension built with another tile shape or pass count, loaded in place of the tree's)"""
import importlib.machinery
import importlib.util
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--lib" in sys.argv[1:]:
    _path = sys.argv[sys.argv.index("--lib") + 1]
    import unet_distributed_amd  # noqa: E402,F401
    _ld = importlib.machinery.ExtensionFileLoader("unet_distributed_amd._C", _path)
    _mod = importlib.util.module_from_spec(importlib.util.spec_from_loader("unet_distributed_amd._C", _ld))
    _ld.exec_module(_mod)
    sys.modules["unet_distributed_amd._C"] = _mod
    unet_distributed_amd._C = _mod
from unet_distributed_amd import native  # noqa: E402
from unet_distributed_amd.data.augment import (apply_torch, draw_elastic, draw_spatial, draw_spatial3, embed_mat3,  # noqa: E402
                                               elastic_torch, mat3_of, warp3_torch, warp_torch)

C = native.require()
dev = torch.device("cuda:0")
CIN = 4
ITERS, REPS, SETS = 100, 3, 4


def run(B, patch, stored, nall, K, fp32, names):
    D, H, W = patch
    dt, pre, cpad = (torch.float32, "f32_", CIN) if fp32 else (torch.bfloat16, "", 4)
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(2)
    x_all = torch.randn((nall,) + tuple(stored) + (CIN,), device=dev, generator=g)
    y_all = (torch.rand((nall,) + tuple(stored) + (K,), device=dev, generator=g) > 0.6).float()
    idxs = [torch.from_numpy(np.sort(rng.choice(nall, B, replace=False))).to(dev) for _ in range(SETS)]
    outs = [(torch.empty((B,) + tuple(patch) + (cpad,), dtype=dt, device=dev),
             torch.empty((B,) + tuple(patch) + (K,), dtype=dt, device=dev)) for _ in range(SETS)]
    st = int(torch.cuda.current_stream().cuda_stream)
    origin = torch.from_numpy(np.stack([rng.integers(0, s - t + 1, B) for s, t in zip(stored, patch)],
                                       axis=1).astype(np.int32)).to(dev)
    mixed = torch.from_numpy(rng.integers(0, 16, B).astype(np.int32)).to(dev)
    zero = torch.zeros_like(mixed)
    one = np.ones(B)
    r30 = np.radians(30.0)
    t = lambda m: torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to(dev)
    m2_eye = t(np.tile([65536, 0, 0, 65536], (B, 1)))
    m2_drawn = t(draw_spatial(3, 7, np.arange(B), "rotate,scale", 30.0, 0.25))
    m3 = {"eye": t(embed_mat3(m2_eye.cpu().numpy())),
          "drawn": t(draw_spatial3(3, 7, np.arange(B), "rotate3d,scale3d", 30.0, 15.0, 0.25)),
          "d30": t(mat3_of(r30 * one, 0, 0, 1, 1)), "h30": t(mat3_of(0, r30 * one, 0, 1, 1)),
          "w30": t(mat3_of(0, 0, r30 * one, 1, 1))}
    f32 = torch.from_numpy(draw_elastic(3, 7, np.arange(B), H, 4.0, 32)).to(dev)
    # case: (op, matrices, codes, field)
    cases = {"warp_identity": ("warp", m2_eye, zero, None), "warp_drawn": ("warp", m2_drawn, zero, None),
             "warp_drawn_mixed": ("warp", m2_drawn, mixed, None),
             "warp3_identity": ("warp3", m3["eye"], zero, None), "warp3_drawn": ("warp3", m3["drawn"], zero, None),
             "warp3_d30": ("warp3", m3["d30"], zero, None), "warp3_h30": ("warp3", m3["h30"], zero, None),
             "warp3_w30": ("warp3", m3["w30"], zero, None), "warp3_drawn_mixed": ("warp3", m3["drawn"], mixed, None),
             "elastic_drawn_mixed": ("elastic", m2_drawn, mixed, f32),
             "warp3_field_identity": ("warp3", m3["eye"], mixed, f32),
             "warp3_field_drawn_mixed": ("warp3", m3["drawn"], mixed, f32),
             "warp3_field_h30": ("warp3", m3["h30"], mixed, f32)}
    cases = {k: cases[k] for k in names}
    ints = [B] + list(stored) + list(patch) + [CIN, cpad, K]

    def launch(case, i):
        j = i % SETS
        xb, tb = outs[j]
        op, mat, code, fld = cases[case]
        head = [x_all.data_ptr(), y_all.data_ptr(), idxs[j].data_ptr(), origin.data_ptr(), code.data_ptr(), mat.data_ptr(), 0]
        tail = [xb.data_ptr(), tb.data_ptr()]
        if op == "warp":
            C.generic(pre + "gather_batch_warp", head + tail, ints, [], st, 0)
        else:
            C.generic(pre + "gather_batch_" + op, head + [fld.data_ptr() if fld is not None else 0] + tail,
                      ints + [5], [], st, 0)

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

    # results first: the first two volumes of the drawn batches against the definition in torch
    bits = torch.int32 if fp32 else torch.int16
    n = 2
    ok = {}
    for chk in [c for c in names if c in ("warp3_drawn_mixed", "warp3_field_drawn_mixed", "warp3_h30")]:
        launch(chk, 0)
        torch.cuda.synchronize()
        sel = idxs[0][:n]
        _, mat, code, fld = cases[chk]
        wx, wt = apply_torch(*warp3_torch(x_all.index_select(0, sel), y_all.index_select(0, sel), origin[:n], patch,
                                          mat[:n], (fld[:n], 32) if fld is not None else None), code[:n])
        ok[chk] = bool(torch.equal(outs[0][0][:n].view(bits), wx.to(dt).view(bits))
                       and torch.equal(outs[0][1][:n].view(bits), wt.to(dt).view(bits)))
        del wx, wt
        torch.cuda.empty_cache()

    rec = dict(B=B, patch=list(patch), stored=list(stored), Cin=CIN, Cpad=cpad, K=K, out="fp32" if fp32 else "bf16",
               iters=ITERS, resident_GB=round((x_all.numel() + y_all.numel()) * 4 / 1e9, 2), matches_torch=ok, us={})
    for rep in range(REPS):
        for case in cases:                          # interleaved: every case once per repetition
            rec["us"].setdefault(case, []).append(round(timeit(case), 2))
    for base in [c for c in ("warp_drawn_mixed", "elastic_drawn_mixed") if c in names]:
        b = rec["us"][base]
        rec["spread_" + base] = round(max(b) / min(b) - 1.0, 4)
        rec["ratio_to_" + base] = {c: round(float(np.median(v) / np.median(b)), 4) for c, v in rec["us"].items()}
    print(json.dumps(rec), flush=True)


ALL = ["warp_identity", "warp_drawn", "warp_drawn_mixed", "warp3_identity", "warp3_drawn", "warp3_d30", "warp3_h30",
       "warp3_w30", "warp3_drawn_mixed", "elastic_drawn_mixed", "warp3_field_identity", "warp3_field_drawn_mixed",
       "warp3_field_h30"]
SHAPE = (8, (128, 128, 128), (155, 240, 240), 16)
run(*SHAPE, 1, False, ALL)
if "--quick" not in sys.argv[1:]:
    torch.cuda.empty_cache()
    run(*SHAPE, 3, False, ALL)
    torch.cuda.empty_cache()
    run(*SHAPE, 1, True, ALL)

"""The conv, data-gradient and weight-gradient kernels against float64 CPU references,
bit for bit (tests/exact_ref.py): integer operands keep every fp32 partial sum exact, so
the stored value must be the round-to-nearest-even image of the mathematical result and
the fp32 slabs must sum to the integer gradient.  The base kernels the variant tests
(persistent / chunk-pipelined window, fused data + weight gradient, ...) compare against
are held to the same equality the variants are.

Each case launches a parameter dict an existing test launches (buffers and operand values
apart) and prints one `EXACT|...` line: case, kernel id, sum |x||w|, rounding shares, ms."""

import collections
import time

import pytest
import torch

import exact_ref as X
from test_gpu_kernels import C, pack_dgrad, pack_fwd, pad64, ptr, stream

pytestmark = pytest.mark.gpu
DT = {"bf16": 0, "fp16": 1}


def S(t, dtype="bf16"):
    return X.to_storage(t, dtype)


def f32(t):
    return X.to_storage(t, "fp32")


def nan16(shape, dtype="bf16"):
    return torch.full(tuple(shape), float("nan"), device="cuda", dtype=X.DTYPES[dtype])


def report(name, pick, case, ref64, t0, rounds=None):
    """rounds=False: an fp32 output (slabs) of a case whose other outputs are 16-bit"""
    rounds = case.rounds if rounds is None else rounds
    nr, tie = X.rounding_share(ref64, case.dtype) if rounds else (0.0, 0.0)
    print("EXACT|%s|%s|%.4g|%.1f|%.1f|%.0f" % (name, pick, case.bound, 100 * nr, 100 * tie, 1e3 * (time.perf_counter() - t0)))


def check16(out, ref64, case, what):
    X.require_exact(case.bound, ref64, case.dtype)
    torch.cuda.synchronize()
    X.assert_bits_equal(out, X.rne(ref64, case.dtype), what, ref64, case.dtype)


def check32(out, ref64, case, what):
    X.require_exact(case.bound)
    torch.cuda.synchronize()
    X.assert_bits_equal(out.reshape(ref64.shape), X.rne(ref64, "fp32"), what, ref64, "fp32")


# ------------------------------------------------------------------------------ forward
def geo(N, D, H, W, k=3):
    g = dict(N=N, OH=H, OW=W, IH=H, IW=W, KH=k, KW=k, pad=1)
    if D > 1:
        g.update(OD=D, ID=D, KD=k)
    return g


def fwd_dict(key, P, relu=1):
    N, D, H, W, C1, C2, Cout, tile = key[:8]
    return dict(geo(N, D, H, W), C1=C1, C2=C2, src1=P["a"], src2=P["b2"] if C2 else None, wgt=P["w"], bias=P["bias"],
                Cout=Cout, relu=relu, dst1=P["y"], tile=tile)


def pack_w(w, dtype):
    """[(kd,) kh, kw, ci, co] -> [co][taps * ci (pad 64)] in the storage type"""
    ws = S(w, dtype)
    return pack_fwd(ws) if w.dim() == 4 else pad64(ws.movedim(-1, 0).reshape(w.shape[-1], -1))


def pack_wd(w, dtype):
    """-> [ci][flipped taps * co (pad 64)]"""
    ws = S(w, dtype)
    if w.dim() == 4:
        return pack_dgrad(ws)
    return pad64(ws.flip(0, 1, 2).permute(3, 0, 1, 2, 4).reshape(w.shape[-2], -1))


def fwd_ptrs(case, dtype, keep):
    o = case.ops
    keep += [S(o["a"], dtype), S(o["b2"], dtype) if o["b2"] is not None else None, pack_w(o["w"], dtype),
             f32(o["bias"])]
    a, b2, w, bias = keep[-4:]
    return dict(a=ptr(a), b2=ptr(b2) if b2 is not None else None, w=ptr(w), bias=ptr(bias))


# variants of one shape that must all write the same bits: the persistent prefetching window
# (5 windows per workgroup, both walk orders) and the chunk-pipelined window
VARIANTS = {(3, 1, 128, 128, 32, 0, 32, 0): [{}, dict(win_pf=5), dict(win_pf=5, rev=1)],
            (3, 1, 64, 64, 64, 0, 64, 0): [{}, dict(win_cp=2)]}
FWD = [("bf16", k) for k in X.FWD_BF16] + [("fp16", k) for k in X.FWD_FP16]


@pytest.mark.parametrize("dtype,key", FWD, ids=["%s-%s" % (d, "x".join(map(str, k))) for d, k in FWD])
def test_forward_bias_relu(cuda_dev, dtype, key):
    t0 = time.perf_counter()
    N, D, H, W, C1, C2, Cout, tile, pick = key
    case = X.fwd_case(N, D, H, W, C1, C2, Cout, dtype)
    keep = []
    P = fwd_ptrs(case, dtype, keep)
    shape = case.ref["y"].shape
    for var in VARIANTS.get(key[:8], [{}]):
        y = nan16(shape, dtype)
        d = dict(fwd_dict(key, dict(P, y=ptr(y))), **var)
        assert C().conv_fwd_pick(d) == pick, (C().conv_fwd_pick(d), pick)
        if var.get("win_pf"):
            assert C().conv_fwd_grid(d) == (N * H // 4 + var["win_pf"] - 1) // var["win_pf"]
        elif pick in (6, 12):
            assert C().conv_fwd_grid(d) > 0
        C().conv_fwd(d, stream(), dtype=DT[dtype])
        check16(y, case.ref["y"], case, "forward %s %s %s" % (dtype, key, var))
    report("fwd %s %s" % (dtype, key[:8]), pick, case, case.ref["y"], t0)


# (N, D, H, W, C1, C2, Cout, tile, expected conv_fwd_pick id)
BITS = [(3, 1, 128, 128, 32, 0, 32, 0, 6), (2, 1, 16, 16, 32, 0, 32, 8, 4), (3, 1, 128, 128, 4, 0, 32, 9, 9),
        (5, 1, 8, 8, 64, 64, 128, 0, 13), (5, 1, 16, 16, 64, 0, 128, 12, 12)]


@pytest.mark.parametrize("key", BITS, ids=["x".join(map(str, k)) for k in BITS])
def test_forward_relu_bit_mask(cuda_dev, key):
    """The 1-bit-per-element ReLU mask a forward writes next to its output, as bytes."""
    t0 = time.perf_counter()
    case = X.fwd_case(*key[:7], "bf16")
    keep = []
    P = fwd_ptrs(case, "bf16", keep)
    ref = case.ref["y"]
    y = nan16(ref.shape)
    bits = torch.full(ref.shape[:-1] + (ref.shape[-1] // 8,), 0xA5, device="cuda", dtype=torch.uint8)
    d = dict(fwd_dict(key, dict(P, y=ptr(y))), relu_bits=ptr(bits))
    assert C().conv_fwd_pick(d) == key[8]
    C().conv_fwd(d, stream())
    check16(y, ref, case, "forward with ReLU bits %s" % (key,))
    X.assert_bits_equal(bits, X.pack_bits(X.rne(ref, "bf16").float()), "ReLU bit mask %s" % (key,))
    report("relu_bits %s" % (key[:8],), key[8], case, ref, t0)


POOL = [((3, 1, 128, 128, 32, 0, 32, 0, 6), {}), ((3, 1, 128, 128, 32, 0, 32, 0, 6), dict(win_pf=5, rev=1)),
        ((3, 1, 64, 64, 64, 0, 64, 0, 6), {}), ((3, 1, 64, 64, 64, 0, 64, 0, 6), dict(win_cp=2)),
        ((5, 1, 16, 16, 64, 0, 128, 12, 12), {})]


@pytest.mark.parametrize("key,var", POOL, ids=["%s-%s" % ("x".join(map(str, k)), "-".join(v) or "plain") for k, v in POOL])
def test_forward_fused_maxpool(cuda_dev, key, var):
    """Fused 2x2 max-pool epilogue: the pooled tensor and the first-argmax codes, the argmax
    taken over the rounded outputs."""
    t0 = time.perf_counter()
    case = X.fwd_case(*key[:7], "bf16")
    keep = []
    P = fwd_ptrs(case, "bf16", keep)
    ref = case.ref["y"]
    stored = X.rne(ref, "bf16").double()
    pooled64, codes = X.pool_ref(stored)
    y = nan16(ref.shape)
    pooled = nan16(pooled64.shape)
    code = torch.full((codes.numel(),), -1, device="cuda", dtype=torch.int32)
    d = dict(fwd_dict(key, dict(P, y=ptr(y))), pool_dst=ptr(pooled), pool_code=ptr(code), **var)
    assert C().conv_fwd_pick(d) == key[8]
    C().conv_fwd(d, stream())
    check16(y, ref, case, "forward with fused pool %s" % (key,))
    X.assert_bits_equal(pooled, X.rne(pooled64, "bf16"), "pooled tensor %s %s" % (key, var), pooled64, "bf16")
    X.assert_bits_equal(code, codes, "argmax codes %s %s" % (key, var))
    report("pool %s %s" % (key[:8], var), key[8], case, ref, t0)


@pytest.mark.parametrize("key", X.STATS, ids=["x".join(map(str, k)) for k in X.STATS])
def test_forward_statistics_rows(cuda_dev, key):
    """Pre-norm z and the {sum z, sum z^2} rows of the stored z: |z| <= 64 and at most 4096
    pixels per sample keep every row an exact integer, so the rows sum to the moments."""
    t0 = time.perf_counter()
    N, D, H, W, C1, C2, Cout, tile, pick = key
    case = X.fwd_case(N, D, H, W, C1, C2, Cout, "bf16", False, True)
    keep = []
    P = fwd_ptrs(case, "bf16", keep)
    z64 = case.ref["y"]
    assert z64.abs().max() <= 64 and H * W <= 4096
    mom = torch.stack([z64.reshape(N, -1, Cout).sum(1), (z64 * z64).reshape(N, -1, Cout).sum(1)], 1)   # [N, 2, C]
    X.require_exact(mom)
    z = nan16(z64.shape)
    d = fwd_dict(key, dict(P, y=ptr(z)), relu=0)
    rows, px = C().conv_stat_tiles(dict(d, stats=1))
    assert rows > 0
    st = torch.full((rows, 2, Cout), float("nan"), device="cuda")
    assert C().conv_fwd_pick(dict(d, stats=ptr(st))) == pick
    C().conv_fwd(dict(d, stats=ptr(st)), stream())
    check16(z, z64, case, "pre-norm z %s" % (key,))
    if (H * W) % px == 0 and rows % N == 0:
        got = st.double().view(N, rows // N, 2, Cout).sum(1)
        X.assert_bits_equal(got, mom, "per-sample statistics rows %s" % (key,))
    else:                       # tiles span samples (8x8 images): the totals
        X.assert_bits_equal(st.double().sum(0), mom.sum(0), "statistics totals %s" % (key,))
    report("stats %s rows=%d px=%d" % (key[:8], rows, px), pick, case, z64, t0)


def test_forward_dropout_half(cuda_dev):
    """Dropout at rate 0.5 (generic epilogue): the keep hash of models/reference._hash_u32, the
    rescale exactly 2."""
    from unet_distributed_amd.models.reference import dropout_keep_mask
    t0 = time.perf_counter()
    key = X.DROPOUT + (0,)
    case = X.fwd_case(*X.DROPOUT)
    keep = []
    P = fwd_ptrs(case, "bf16", keep)
    ref = case.ref["y"]
    keepm = dropout_keep_mask(1234, 7, tuple(ref.shape), 0.5, torch.device("cpu"))
    assert 0 < keepm.sum() < keepm.numel()
    ref = ref * keepm.double() * 2.0
    y = nan16(ref.shape)
    # (the dict of test_dropout_matches_reference_hash plus a bias, so that the bias is seen to
    # be added before the rescale)
    d = dict(fwd_dict(key, dict(P, y=ptr(y))), drop_rate=0.5, seed=1234, salt=7)
    d.pop("tile")
    assert C().conv_fwd_pick(d) == X.DROPOUT_PICK
    C().conv_fwd(d, stream())
    X.require_exact(2 * case.bound)
    check16(y, ref, case, "dropout 0.5 forward")
    report("dropout %s" % (key,), X.DROPOUT_PICK, case, ref, t0)


@pytest.mark.parametrize("pf,rev", [(0, 0), (5, 1)])
def test_forward_fused_head_logit(cuda_dev, pf, rev):
    """The fused segmentation head's fp32 logit: integer head weights dotted with the stored
    (rounded) activations, no sigmoid."""
    t0 = time.perf_counter()
    key = (3, 1, 128, 128, 32, 0, 32, 0)
    case = X.fwd_case(*key[:7], "bf16")
    keep = []
    P = fwd_ptrs(case, "bf16", keep)
    ref = case.ref["y"]
    hw64 = X.ints(77, (32,), -4, 4)
    hb64 = torch.tensor([3.0], dtype=torch.float64)
    stored = X.rne(ref, "bf16").double()
    logit64 = stored.reshape(-1, 32) @ hw64 + hb64
    X.require_exact(stored.reshape(-1, 32).abs() @ hw64.abs() + hb64.abs())
    hw, hb = f32(hw64), f32(hb64)
    y = nan16(ref.shape)
    bits = torch.zeros(ref.numel() // 8, device="cuda", dtype=torch.uint8)
    logit = torch.full((logit64.numel(),), float("nan"), device="cuda")
    d = dict(fwd_dict(key, dict(P, y=ptr(y))), head_w=ptr(hw), head_b=ptr(hb), head_logit=ptr(logit),
             relu_bits=ptr(bits), win_pf=pf, rev=rev)
    assert C().conv_fwd_pick(d) == 6
    C().conv_fwd(d, stream())
    check16(y, ref, case, "forward with fused head")
    X.assert_bits_equal(logit, X.rne(logit64, "fp32"), "head logit", None)
    X.assert_bits_equal(bits, X.pack_bits(stored).reshape(-1), "ReLU bits with fused head")
    report("head logit pf=%d rev=%d" % (pf, rev), 6, case, ref, t0)


# --------------------------------------------------------------------- transposed conv
def tconv_dicts(N, H, Ci, Co, tile, P):
    fwd = dict(N=N, OH=H, OW=H, IH=H, IW=H, C1=Ci, src1=P["x"], wgt=P["wf"], bias=P["bias"], Cout=4 * Co, shuffle=2,
               dst1=P["y"], tile=tile)
    dg = dict(N=N, OH=H, OW=H, IH=2 * H, IW=2 * H, KH=2, KW=2, stride=2, pad=0, C1=Co, src1=P["dout"], wgt=P["wd"],
              Cout=Ci, dst1=P["dx"], mask1=P["x"], tile=tile)
    return fwd, dg


# (N, H, Ci, Co, tile, expected ids of the forward and the data gradient)
TCONV = [(2, 8, 64, 32, 0, (10, 11)), (2, 8, 64, 32, 8, (2, 2)), (3, 64, 64, 32, 0, (10, 11))]


@pytest.mark.parametrize("N,H,Ci,Co,tile,picks", TCONV)
def test_tconv_forward_and_data_gradient(cuda_dev, N, H, Ci, Co, tile, picks):
    """2x2 stride-2 transposed conv with its pixel shuffle (window kernels and implicit GEMM)
    and its data gradient with the x > 0 mask."""
    t0 = time.perf_counter()
    case = X.tconv_case(N, 1, H, Ci, Co)
    o = case.ops
    x, k, bias, dout = S(o["x"]), S(o["k"]), f32(o["bias"]), S(o["dout"])
    wf = pad64(k.reshape(4 * Co, Ci))
    wd = pad64(k.permute(3, 0, 1, 2).reshape(Ci, 4 * Co))
    y, dx = nan16(case.ref["y"].shape), nan16(case.ref["dx"].shape)
    fwd, dg = tconv_dicts(N, H, Ci, Co, tile, dict(x=ptr(x), wf=ptr(wf), wd=ptr(wd), bias=ptr(bias), dout=ptr(dout),
                                                  y=ptr(y), dx=ptr(dx)))
    pf, pd = C().conv_fwd_pick(fwd), C().conv_fwd_pick(dg)
    assert (pf, pd) == picks
    C().conv_fwd(fwd, stream())
    check16(y, case.ref["y"], case, "tconv forward %s" % ((N, H, Ci, Co, tile),))
    C().conv_fwd(dg, stream())
    check16(dx, case.ref["dx"], case, "tconv data gradient %s" % ((N, H, Ci, Co, tile),))
    report("tconv fwd %s" % ((N, H, Ci, Co, tile),), pf, case, case.ref["y"], t0)
    report("tconv dgrad %s" % ((N, H, Ci, Co, tile),), pd, case, case.ref["dx"], t0)


# -------------------------------------------------------------------- data gradients
def dgrad_dict(N, D, H, C1, C2, Co, tile, P, bits, scale2):
    d = dict(geo(N, D, H, H), C1=Co, src1=P["dy"], wgt=P["w"], Cout=C1 + C2, D1=C1, dst1=P["d1"], dst2=P["d2"],
             mask2=P["m2"], tile=tile)
    if D == 1:
        d.update(mask1=P["m1"], mask_scale2=scale2)
    if bits:
        d.update(mask_bits=3)
    return d


DGRAD = [((2, 1, 16, 32, 32, 32, "bf16"), 8, False, 2), ((2, 1, 16, 32, 32, 32, "bf16"), 8, True, 2),
         ((2, 1, 128, 32, 32, 32, "bf16"), 6, False, 6), ((2, 1, 128, 32, 32, 32, "bf16"), 6, True, 6),
         ((2, 1, 128, 32, 32, 32, "bf16"), 8, False, 2), ((2, 1, 128, 32, 32, 32, "bf16"), 8, True, 2),
         ((2, 1, 128, 32, 32, 32, "bf16"), 12, False, 12), ((2, 1, 128, 32, 32, 32, "bf16"), 12, True, 12),
         ((6, 1, 8, 256, 256, 512, "bf16"), 0, True, 13),
         ((2, 3, 64, 32, 32, 32, "bf16"), 6, False, 6),
         ((2, 1, 16, 32, 32, 32, "fp16"), 6, False, 6)]


@pytest.mark.parametrize("key,tile,bits,picks", DGRAD,
                         ids=["%s-t%d-%s" % ("x".join(map(str, k)), t, "bits" if b else "act") for k, t, b, _ in DGRAD])
def test_data_gradient_dual_destination(cuda_dev, key, tile, bits, picks):
    # (picks: the one expected conv_fwd_pick id)
    """Concat conv data gradient: flipped weights, two destinations, ReLU masks from the
    activations or from 1-bit masks, the second half rescaled by 1.25 (exact in fp32)."""
    t0 = time.perf_counter()
    N, D, H, C1, C2, Co, dtype = key
    case = X.dgrad_case(N, D, H, H, C1, C2, Co, dtype)
    o = case.ops
    dy, w = S(o["dy"], dtype), pack_wd(o["w"], dtype)
    m1 = X.pack_bits(o["m1"]).cuda() if bits else S(o["m1"], dtype)
    m2 = X.pack_bits(o["m2"]).cuda() if bits else S(o["m2"], dtype)
    d1, d2 = nan16(case.ref["d1"].shape, dtype), nan16(case.ref["d2"].shape, dtype)
    d = dgrad_dict(N, D, H, C1, C2, Co, tile, dict(dy=ptr(dy), w=ptr(w), m1=ptr(m1), m2=ptr(m2), d1=ptr(d1), d2=ptr(d2)),
                   bits, 1.25)
    pick = C().conv_fwd_pick(d)
    assert pick == picks, (pick, picks)
    C().conv_fwd(d, stream(), dtype=DT[dtype])
    check16(d1, case.ref["d1"], case, "data gradient, first destination %s tile %d" % (key, tile))
    check16(d2, case.ref["d2"], case, "data gradient, second destination %s tile %d" % (key, tile))
    report("dgrad %s tile=%d bits=%d d1" % (key, tile, bits), pick, case, case.ref["d1"], t0)
    report("dgrad %s tile=%d bits=%d d2" % (key, tile, bits), pick, case, case.ref["d2"], t0)


@pytest.mark.parametrize("key", X.ROUTE)
def test_data_gradient_skip_half_with_pool_backward(cuda_dev, key):
    """The decoder conv's data gradient in two launches: the upsampled half, and the skip half
    with the max-pool backward in its epilogue: RNE(RNE(masked conv) + routed gy)."""
    t0 = time.perf_counter()
    N, H, C1, C2, Co = key
    case = X.pool_route_case(*key)
    o = case.ops
    dy, wdg, gy = S(o["dy"]), pack_wd(o["w"], "bf16"), S(o["gy"])
    bits = X.pack_bits(o["y"]).cuda()
    _, codes64 = X.pool_ref(o["y"])
    codes = codes64.cuda()
    g = dict(geo(N, 1, H, H), C1=Co, src1=ptr(dy))
    d_up, d_skip = nan16(case.ref["up"].shape), nan16(case.ref["skip"].shape)
    du = dict(g, wgt=ptr(wdg), Cout=C1, dst1=ptr(d_up))
    ds = dict(g, wgt=ptr(wdg) + 2 * C1 * wdg.shape[1], Cout=C2, dst1=ptr(d_skip), mask1=ptr(bits), mask_bits=1,
              route_gy=ptr(gy), pool_code=ptr(codes))
    assert C().conv_fwd_pick(du) == 6 and C().conv_fwd_pick(ds) == 6
    C().conv_fwd(du, stream())
    C().conv_fwd(ds, stream())
    check16(d_up, case.ref["up"], case, "upsampled half %s" % (key,))
    final = X.route_final(case)
    assert case.ref["routed"].abs().sum() > 0
    check16(d_skip, final, case, "skip half + routed pool gradient %s" % (key,))
    report("route %s" % (key,), 6, case, final, t0)


# ------------------------------------------------------------- linear on-load transforms
@pytest.mark.parametrize("N,H,Cin,Cout,gn,tile,stats", X.NORM_ONLOAD)
def test_normalise_on_load_forward(cuda_dev, N, H, Cin, Cout, gn, tile, stats):
    """xform 1: relu(a z + b) formed in LDS (16 bits by design) with integer coefficients, the
    conv of it rounded once; xout holds the activation."""
    t0 = time.perf_counter()
    case = X.norm_onload_case(N, H, Cin, Cout, gn)
    o = case.ops
    z, a, b, w, bias = S(o["z"]), f32(o["a"]), f32(o["b"]), pack_w(o["w"], "bf16"), f32(o["bias"])
    out, yo = nan16(case.ref["out"].shape), nan16(case.ref["_y"].shape)
    d = dict(geo(N, 1, H, H), C1=Cin, src1=ptr(z), wgt=ptr(w), bias=ptr(bias), Cout=Cout, relu=0, dst1=ptr(out),
             tile=tile, xform=1, xa=ptr(a), xb=ptr(b), xcs=Cin if gn else 0, xout=ptr(yo))
    if stats:
        nr, _ = C().conv_stat_tiles(dict(d, stats=1))
        st = torch.zeros(nr, 2, Cout, device="cuda")
        d["stats"] = ptr(st)
    pick = C().conv_fwd_pick(d)
    assert pick == 6
    C().conv_fwd(d, stream())
    check16(out, case.ref["out"], case, "conv of the activation normalised on load")
    X.assert_bits_equal(yo, S(case.ref["_y"]).cpu(), "xout", case.ref["_y"], "bf16")
    report("norm on load %s" % ((N, H, Cin, Cout, gn, tile, stats),), pick, case, case.ref["out"], t0)


@pytest.mark.parametrize("N,W,Co,Ci,gn", X.DZ_ONLOAD)
def test_dz_on_load_data_gradient(cuda_dev, N, W, Co, Ci, gn):
    """xform 2: the data gradient's halo dz = ca g + cb z + cc formed on load."""
    t0 = time.perf_counter()
    case = X.dz_onload_case(N, W, Co, Ci, gn)
    o = case.ops
    g, z, act, w = S(o["g"]), S(o["z"]), S(o["act"]), pack_wd(o["w"], "bf16")
    ca, cb, cc = f32(o["ca"]), f32(o["cb"]), f32(o["cc"])
    dx = nan16(case.ref["dx"].shape)
    d = dict(geo(N, 1, W, W), C1=Co, wgt=ptr(w), Cout=Ci, relu=0, mask1=ptr(act), src1=ptr(g), xform=2, xa=ptr(ca),
             xb=ptr(cb), xc=ptr(cc), xz=ptr(z), xcs=Co if gn else 0, dst1=ptr(dx))
    pick = C().conv_fwd_pick(d)
    assert pick == 6
    C().conv_fwd(d, stream())
    check16(dx, case.ref["dx"], case, "data gradient with dz formed on load %s" % ((N, W, Co, Ci, gn),))
    report("dz on load %s" % ((N, W, Co, Ci, gn),), pick, case, case.ref["dx"], t0)


def tconv_onload_run(key, pf, rev):
    N, H, K, Cc, Cs, O = key
    case = X.tconv_onload_case(*key)
    o = case.ops
    F2 = 2 * H
    b, skip, bt, ba = S(o["b"]), S(o["skip"]), f32(o["bt"]), f32(o["ba"])
    wtp = pad64(S(o["wt"]).reshape(4 * Cc, K))
    wap = pack_w(o["wa"], "bf16")
    z = nan16(case.ref["z"].shape)
    bits = torch.zeros(N * F2 * F2 * O // 8, device="cuda", dtype=torch.uint8)
    d = dict(geo(N, 1, F2, F2), C1=Cc, C2=Cs, src1=ptr(b), src2=ptr(skip), wgt=ptr(wap), bias=ptr(ba), Cout=O, relu=1,
             dst1=ptr(z), relu_bits=ptr(bits), ut_x=ptr(b), ut_w=ptr(wtp), ut_b=ptr(bt), ut_C=K, ut_kpad=wtp.shape[1])
    if pf:
        d.update(win_pf=pf, rev=rev)
        assert C().conv_fwd_grid(d) == (N * F2 // 2 + pf - 1) // pf
    pick = C().conv_fwd_pick(d)
    assert pick == 6
    C().conv_fwd(d, stream())
    check16(z, case.ref["z"], case, "conv of [u formed on load, skip] %s pf=%d" % (key, pf))
    X.assert_bits_equal(bits, X.pack_bits(case.ref["z"]).reshape(-1), "ReLU bits %s pf=%d" % (key, pf))
    return pick, case


@pytest.mark.parametrize("key", X.TCONV_ONLOAD)
def test_tconv_on_load_forward(cuda_dev, key):
    """z = relu(conv3x3([u, skip]) + ba), u = RNE(tconv(b) + bt) formed on load."""
    t0 = time.perf_counter()
    pick, case = tconv_onload_run(key, 0, 0)
    report("tconv on load %s" % (key,), pick, case, case.ref["z"], t0)


@pytest.mark.parametrize("key", X.TCONV_ONLOAD_PF)
def test_tconv_on_load_persistent_window(cuda_dev, key):
    t0 = time.perf_counter()
    pick, case = tconv_onload_run(key[:6], key[6], key[7])
    report("tconv on load, persistent %s" % (key,), pick, case, case.ref["z"], t0)


@pytest.mark.parametrize("key", X.S2D)
def test_composite_tconv_data_gradient(cuda_dev, key):
    """db = S2D(dz) (*) compose(Wt, Wa), masked by the ReLU bits of b: the true chain-rule
    gradient, rounded once (|wt|, |wa| <= 1: the composed 16-bit weights are exact)."""
    t0 = time.perf_counter()
    N, H, K, Cc, Cs, O = key
    case = X.s2d_case(*key)
    o = case.ops
    b, dz, wt, wa = S(o["b"]), S(o["dz"]), f32(o["wt"]), f32(o["wa"])
    rs = (36 * O + 63) // 64 * 64
    wg = torch.empty(K, rs, device="cuda", dtype=torch.bfloat16)
    C().generic("tconv_compose", [ptr(wt.reshape(4, Cc, K).contiguous()), ptr(wa), ptr(wg)], [Cc, K, O, Cc + Cs, rs], [],
                stream())
    torch.cuda.synchronize()
    assert wg[:, :36 * O].float().abs().max() <= 64
    bits = X.pack_bits(o["b"]).cuda()
    db = nan16(case.ref["db"].shape)
    d = dict(geo(N, 1, H, H), C1=4 * O, s2d=O, src1=ptr(dz), wgt=ptr(wg), Cout=K, dst1=ptr(db), mask1=ptr(bits),
             mask_bits=1)
    pick = C().conv_fwd_pick(d)
    assert pick == 6
    C().conv_fwd(d, stream())
    check16(db, case.ref["db"], case, "composite tconv data gradient %s" % (key,))
    report("s2d dgrad %s" % (key,), pick, case, case.ref["db"], t0)


# ------------------------------------------------------------------ weight gradients
def run_wgrad(d, splits, taps, Mtot, Mout, Nc, bias_w, rows=None, parts=((0, 0),), dtype="bf16"):
    """The launch(es) + the fixed-order slab reduction (test_gpu_kernels._wgrad, with split
    ranges and the storage type)."""
    slab = torch.full((splits * taps * Mtot * Nc,), float("nan"), device="cuda")
    bslab = torch.zeros(splits * 8 * max(Mtot, Nc, 64), device="cuda")
    for lo, n in parts:
        C().wgrad(dict(d, splits=splits, split_lo=lo, split_n=n, slab=ptr(slab), bias_slab=ptr(bslab)), stream(),
                  dtype=DT[dtype])
    out = torch.full((taps * Mout * Nc,), float("nan"), device="cuda")
    stage = torch.zeros(C().wgrad_reduce_stage_floats(max(splits, 64), taps, Mtot, Nc) + 4096, device="cuda")
    ints = [splits, taps, Mtot, Mout, Nc] + (list(rows) if rows else [])
    C().generic("wgrad_reduce", [ptr(slab), ptr(out), ptr(stage)], ints, [1.0], stream())
    nrows, w = bias_w
    bout = torch.full((w,), float("nan"), device="cuda")
    C().generic("wgrad_reduce", [ptr(bslab), ptr(bout), ptr(stage)], [nrows, 1, 1, 1, w], [1.0], stream())
    torch.cuda.synchronize()
    return out, bout


def wgrad_dict(N, D, H, W, C1, C2, Cout, win, P):
    d = dict(N=N, QH=H, QW=W, AH=H, AW=W, KH=3, KW=3, pad=1, M1=C1, M2=C2, a1=P["a"], a2=P["b2"] if C2 else None,
             b=P["dy"], Nc=Cout, bias_mode=1, win=win)
    if D > 1:
        d.update(QD=D, AD=D, KD=3)
    return d


@pytest.mark.parametrize("key", X.WGRAD, ids=["x".join(map(str, k)) for k in X.WGRAD])
def test_weight_and_bias_gradient(cuda_dev, key):
    """fp32 slabs: the sum after the fixed-order reduction is the integer gradient -- tiled and
    row-window kernels, more splits than windows, concat sources, segmented rows, 3D, the first
    layer (padded channels dropped by the row remap), bf16 and fp16."""
    t0 = time.perf_counter()
    N, D, H, W, C1, C2, Cout, splits, win, creal, dtype, expect = key
    case = X.wgrad_case(N, D, H, W, C1, C2, Cout, dtype, creal)
    o = case.ops
    a, b2, dy = S(o["a"], dtype), S(o["b2"], dtype) if C2 else None, S(o["dy"], dtype)
    d = wgrad_dict(N, D, H, W, C1, C2, Cout, win, dict(a=ptr(a), b2=ptr(b2) if C2 else None, dy=ptr(dy)))
    T = 27 if D > 1 else 9
    kw = dict(QW=W, QH=H, win=win)
    if D > 1:
        kw.update(QD=D)
    pick = tuple(C().wgrad_pick(C1, C2, Cout, T, **kw))
    assert pick == expect, (pick, expect)
    if creal:
        Mtot = (T * C1 + pick[0] - 1) // pick[0] * pick[0]
        gw, gb = run_wgrad(d, splits, 1, Mtot, T * creal, Cout, (splits, Cout), rows=(C1, creal), dtype=dtype)
    else:
        Mt = C1 + C2
        gw, gb = run_wgrad(d, splits, T, Mt, Mt, Cout, (splits, Cout), dtype=dtype)
    check32(gw, case.ref["gw"], case, "weight gradient %s" % (key,))
    check32(gb, case.ref["gb"], case, "bias gradient %s" % (key,))
    report("wgrad %s" % (key[:11],), "wgrad_pick=%s" % (pick,), case, case.ref["gw"], t0)


def test_weight_gradient_prefetching_window(cuda_dev):
    t0 = time.perf_counter()
    N, D, H, W, C1, C2, Cout, splits, expect = X.WGRAD_PF
    assert tuple(C().wgrad_pick(C1, C2, Cout, 9, QW=W, QH=H, win=0)) == expect
    case = X.wgrad_case(N, D, H, W, C1, C2, Cout)
    o = case.ops
    a, dy = S(o["a"]), S(o["dy"])
    d = dict(N=N, QD=1, QH=H, QW=W, AD=1, AH=H, AW=W, KD=1, KH=3, KW=3, pad=1, M1=C1, M2=0, a1=ptr(a), a2=None,
             b=ptr(dy), Nc=Cout, bias_mode=1)
    for pf in (0, 1):
        gw, gb = run_wgrad(dict(d, pf=pf), splits, 9, C1, C1, Cout, (splits, Cout))
        check32(gw, case.ref["gw"], case, "weight gradient pf=%d" % pf)
        check32(gb, case.ref["gb"], case, "bias gradient pf=%d" % pf)
    report("wgrad pf128 %s" % (X.WGRAD_PF[:8],), "wgrad_pick=%s pf=0,1" % (expect,), case, case.ref["gw"], t0)


@pytest.mark.parametrize("N,H,Ci,Co,splits,expect", X.TCONV_WGRAD)
def test_tconv_weight_and_bias_gradient(cuda_dev, N, H, Ci, Co, splits, expect):
    """bias_mode 2: A = the fine gradient, B = the layer input."""
    t0 = time.perf_counter()
    case = X.tconv_case(N, 1, H, Ci, Co)
    x, dout = S(case.ops["x"]), S(case.ops["dout"])
    d = dict(N=N, QH=H, QW=H, AH=2 * H, AW=2 * H, KH=2, KW=2, stride=2, pad=0, M1=Co, a1=ptr(dout), b=ptr(x), Nc=Ci,
             bias_mode=2, win=0)
    pick = tuple(C().wgrad_pick(Co, 0, Ci, 4, QW=H, win=0))
    assert pick == expect, (pick, expect)
    tg = 4 // pick[2]
    gw, gb = run_wgrad(d, splits, 4, Co, Co, Ci, (splits * tg, Co))
    check32(gw, case.ref["gk"], case, "tconv weight gradient")
    check32(gb, case.ref["gb"], case, "tconv bias gradient")
    report("tconv wgrad %s" % ((N, H, Ci, Co, splits),), "wgrad_pick=%s" % (pick,), case, case.ref["gk"], t0, rounds=False)


@pytest.mark.parametrize("N,H,K,Cc,Cs,O,splits,win", X.TCONV_CHAIN)
def test_composite_tconv_weight_gradients(cuda_dev, N, H, K, Cc, Cs, O, splits, win):
    """The space-to-depth slab sums Hs / Bs, and tconv_chain's dWt, dbt and dWa (u rows through
    Wt, bt; skip rows copied): exact integers."""
    t0 = time.perf_counter()
    case = X.tconv_chain_case(N, H, K, Cc, Cs, O)
    o, r = case.ops, case.ref
    b, dz, wt, bt, wa = S(o["b"]), S(o["dz"]), f32(o["wt"]), f32(o["bt"]), f32(o["wa"])
    slab = torch.full((splits * 16 * O * K,), float("nan"), device="cuda")
    bslab = torch.zeros(splits * 16 * O, device="cuda")
    C().wgrad(dict(N=N, QD=1, QH=H, QW=H, AD=1, AH=2 * H, AW=2 * H, KD=1, KH=4, KW=4, stride=2, pad=1, a1=ptr(dz),
                   b=ptr(b), M1=O, M2=0, Nc=K, splits=splits, slab=ptr(slab), bias_slab=ptr(bslab), bias_mode=2,
                   win=win), stream())
    Hs = torch.full((16 * O * K,), float("nan"), device="cuda")
    Bs = torch.full((16 * O,), float("nan"), device="cuda")
    stage = torch.zeros(C().wgrad_reduce_stage_floats(max(splits, 64), 16, O, K) + 4096, device="cuda")
    C().generic("wgrad_reduce", [ptr(slab), ptr(Hs), ptr(stage)], [splits, 16, O, O, K], [1.0], stream())
    C().generic("wgrad_reduce", [ptr(bslab), ptr(Bs), ptr(stage)], [splits, 1, 1, 1, 16 * O], [1.0], stream())
    check32(Hs, r["Hs"], case, "slab sums Hs")
    check32(Bs, r["Bs"], case, "per-tap bias sums Bs")
    dwt = torch.full((4, Cc, K), float("nan"), device="cuda")
    dbt = torch.full((Cc,), float("nan"), device="cuda")
    C().generic("tconv_chain", [ptr(Hs), ptr(Bs), ptr(wa), ptr(dwt), ptr(dbt)], [Cc, K, O, Cc + Cs], [], stream())
    check32(dwt, r["dwt"], case, "tconv_chain dWt")
    check32(dbt, r["dbt"], case, "tconv_chain dbt")
    dwa = torch.full((3, 3, Cc + Cs, O), float("nan"), device="cuda")
    skg = f32(r["dwa"][:, :, Cc:, :])
    C().generic("tconv_chain", [ptr(Hs), ptr(Bs), ptr(wa), ptr(dwt), ptr(dbt), ptr(wt.reshape(4, Cc, K).contiguous()),
                                ptr(bt), ptr(skg), ptr(dwa)], [Cc, K, O, Cc + Cs], [], stream())
    check32(dwa, r["dwa"], case, "tconv_chain dWa")
    report("tconv chain %s" % ((N, H, K, Cc, Cs, O, splits, win),), "wgrad + tconv_chain", case, r["dwt"], t0)


@pytest.mark.parametrize("kind", ["first", "win", "tconv"])
def test_weight_gradient_split_ranges_compose(cuda_dev, kind):
    """A weight gradient issued in parts (split_lo / split_n) sums to the same integers."""
    t0 = time.perf_counter()
    N, H, splits = 4, 32, 6
    M1, Nc, T = dict(first=(4, 32, 9), win=(64, 64, 9), tconv=(32, 64, 4))[kind]
    pick = tuple(C().wgrad_pick(M1, 0, Nc, T, QW=H, QH=H, win=0))           # (win = 0: the launch's default)
    assert pick == X.SPLIT_PICKS[kind], (pick, X.SPLIT_PICKS[kind])
    for parts in ([(0, 0)], [(0, 3), (3, 3)], [(0, 2), (2, 1), (3, 0)]):
        if kind == "first":
            case = X.wgrad_case(*X.SPLIT_RANGES["first"])
            a, dy = S(case.ops["a"]), S(case.ops["dy"])
            d = wgrad_dict(N, 1, H, H, 4, 0, 32, 0, dict(a=ptr(a), dy=ptr(dy)))
            d.pop("win")
            Mtot = (36 + pick[0] - 1) // pick[0] * pick[0]
            gw, gb = run_wgrad(d, splits, 1, Mtot, 36, 32, (splits, 32), rows=(4, 4), parts=parts)
            ref = case.ref["gw"]
        elif kind == "win":
            case = X.wgrad_case(*X.SPLIT_RANGES["win"])
            a, dy = S(case.ops["a"]), S(case.ops["dy"])
            d = wgrad_dict(N, 1, H, H, 64, 0, 64, 0, dict(a=ptr(a), dy=ptr(dy)))
            d.pop("win")
            gw, gb = run_wgrad(d, splits, 9, 64, 64, 64, (splits, 64), parts=parts)
            ref = case.ref["gw"]
        else:
            case = X.tconv_case(*X.SPLIT_RANGES["tconv"])
            x, dout = S(case.ops["x"]), S(case.ops["dout"])
            d = dict(N=N, QH=H, QW=H, AH=2 * H, AW=2 * H, KH=2, KW=2, stride=2, pad=0, M1=32, a1=ptr(dout), b=ptr(x),
                     Nc=64, bias_mode=2)
            gw, gb = run_wgrad(d, splits, 4, 32, 32, 64, (splits * (4 // pick[2]), 32),
                               parts=parts)
            ref = case.ref["gk"]
        check32(gw, ref, case, "weight gradient in parts %s %s" % (kind, parts))
        check32(gb, case.ref["gb"], case, "bias gradient in parts %s %s" % (kind, parts))
    report("wgrad split ranges %s" % kind, "wgrad_pick=%s" % (pick,), case, ref, t0, rounds=False)


# ------------------------------------------------- fused data + weight gradient (id 14)
def conv_dw_dict(N, nsplit, mask, P):
    d = dict(geo(N, 1, 128, 128), C1=32, src1=P["dy"], wgt=P["w"], Cout=32, relu=0, dst1=P["dx"], fw_x=P["x"],
             fw_slab=P["slab"], fw_bias_slab=P["bslab"], fw_Cx=32, fw_nsplit=nsplit, fw_split_lo=3)
    d.update(dict(mask1=P["mask"]) if mask == "act" else dict(mask1=P["mask"], mask_bits=1))
    return d


@pytest.mark.parametrize("N,nsplit,mask", X.CONV_DW)
def test_fused_data_and_weight_gradient(cuda_dev, N, nsplit, mask):
    """conv_dw: its dx, and its slab rows summing to the integer weight / bias gradient; the
    rows below fw_split_lo stay untouched."""
    t0 = time.perf_counter()
    case = X.conv_dw_case(N, nsplit)
    o = case.ops
    dy, x, w = S(o["dy"]), S(o["x"]), pack_wd(o["w"], "bf16")
    mk = S(o["act"]) if mask == "act" else X.pack_bits(o["act"]).cuda()
    dx = nan16(case.ref["dx"].shape)
    slab = torch.full((nsplit + 3, 9, 32, 32), float("nan"), device="cuda")
    bslab = torch.full((nsplit + 3, 32), float("nan"), device="cuda")
    d = conv_dw_dict(N, nsplit, mask, dict(dy=ptr(dy), w=ptr(w), dx=ptr(dx), x=ptr(x), slab=ptr(slab), bslab=ptr(bslab),
                                           mask=ptr(mk)))
    assert C().conv_fwd_pick(d) == 14 and C().conv_fwd_grid(d) == nsplit
    C().conv_fwd(d, stream())
    check16(dx, case.ref["dx"], case, "fused kernel's data gradient")
    assert torch.isnan(slab[:3]).all() and torch.isnan(bslab[:3]).all()
    X.assert_bits_equal(slab[3:].double().sum(0), case.ref["gw"].reshape(9, 32, 32), "fused kernel's weight gradient")
    X.assert_bits_equal(bslab[3:].double().sum(0), case.ref["gb"], "fused kernel's bias gradient")
    report("conv_dw %s" % ((N, nsplit, mask),), 14, case, case.ref["dx"], t0)


# ------------------------------------------------------------------------ fp32 executor
def f32_transpose(w, T, A, B, flip):
    out = torch.empty(T * A * B, device="cuda")
    C().generic("f32_transpose", [ptr(w), ptr(out)], [T, A, B, int(flip)], [], stream())
    return out


@pytest.mark.parametrize("N,H,C1,C2,Co", X.F32_FWD)
def test_f32_forward(cuda_dev, N, H, C1, C2, Co):
    t0 = time.perf_counter()
    case = X.fwd_case(N, 1, H, H, C1, C2, Co, "fp32", C1 != 1)
    o = case.ops
    a, b = f32(o["a"]), f32(o["b2"]) if C2 else None
    w, bias = f32(o["w"]), f32(o["bias"])
    out = torch.full(tuple(case.ref["y"].shape), float("nan"), device="cuda")
    C().f32_conv(dict(geo(N, 1, H, H), C1=C1, C2=C2, src1=ptr(a), src2=ptr(b) if C2 else None, wgt=ptr(w),
                      bias=ptr(bias), Cout=Co, relu=int(C1 != 1), dst1=ptr(out)), stream())
    check32(out, case.ref["y"], case, "fp32 forward")
    report("f32 fwd %s" % ((N, H, C1, C2, Co),), "f32_conv", case, case.ref["y"], t0)


@pytest.mark.parametrize("C1,C2,Co", X.F32_BWD)
def test_f32_data_and_weight_gradient(cuda_dev, C1, C2, Co):
    t0 = time.perf_counter()
    N, H = 2, 32
    case = X.f32_bwd_case(C1, C2, Co)
    o = case.ops
    xa, xb, w, dy = f32(o["xa"]), f32(o["xb"]), f32(o["w"]), f32(o["dy"])
    wd = f32_transpose(w.reshape(-1), 9, C1 + C2, Co, True)
    mask = torch.cat([xa, xb], -1).contiguous()
    dx = torch.full((N, H, H, C1 + C2), float("nan"), device="cuda")
    C().f32_conv(dict(geo(N, 1, H, H), C1=Co, src1=ptr(dy), wgt=ptr(wd), Cout=C1 + C2, dst1=ptr(dx), mask1=ptr(mask)),
                 stream())
    check32(dx, case.ref["dx"], case, "fp32 data gradient")
    splits = 5
    slab = torch.full((splits, 9, C1 + C2, Co), float("nan"), device="cuda")
    C().f32_wgrad(dict(N=N, QH=H, QW=H, AH=H, AW=H, KH=3, KW=3, pad=1, M1=C1, M2=C2, Nc=Co, a1=ptr(xa), a2=ptr(xb),
                       b=ptr(dy), slab=ptr(slab), splits=splits), stream())
    torch.cuda.synchronize()
    X.assert_bits_equal(slab.double().sum(0), case.ref["gw"].reshape(9, C1 + C2, Co), "fp32 weight gradient")
    report("f32 bwd %s" % ((C1, C2, Co),), "f32_conv/f32_wgrad", case, case.ref["dx"], t0)


@pytest.mark.parametrize("dims", [2, 3])
def test_f32_tconv(cuda_dev, dims):
    t0 = time.perf_counter()
    N, Hc, Ci, Co = 2, 8, 64, 32
    T = 2 ** dims
    case = X.tconv_case(N, Hc if dims == 3 else 1, Hc, Ci, Co, "fp32")
    o = case.ops
    x, wt, bias, gf = f32(o["x"]), f32(o["k"]), f32(o["bias"]), f32(o["dout"])
    wf = f32_transpose(wt.reshape(-1), 1, T * Co, Ci, False)
    out = torch.full(tuple(case.ref["y"].shape), float("nan"), device="cuda")
    d = dict(N=N, OH=Hc, OW=Hc, IH=Hc, IW=Hc, KH=1, KW=1, C1=Ci, src1=ptr(x), wgt=ptr(wf), bias=ptr(bias), Cout=T * Co,
             shuffle=dims, dst1=ptr(out))
    if dims == 3:
        d.update(OD=Hc, ID=Hc)
    C().f32_conv(d, stream())
    check32(out, case.ref["y"], case, "fp32 tconv forward")
    dx = torch.full(tuple(x.shape), float("nan"), device="cuda")
    d = dict(N=N, OH=Hc, OW=Hc, IH=2 * Hc, IW=2 * Hc, KH=2, KW=2, stride=2, pad=0, C1=Co, src1=ptr(gf), wgt=ptr(wt),
             Cout=Ci, dst1=ptr(dx))
    if dims == 3:
        d.update(OD=Hc, ID=2 * Hc, KD=2)
    C().f32_conv(d, stream())
    check32(dx, case.ref["dxu"], case, "fp32 tconv data gradient")
    splits = 3
    slab = torch.full((splits, T, Co, Ci), float("nan"), device="cuda")
    d = dict(N=N, QH=Hc, QW=Hc, AH=2 * Hc, AW=2 * Hc, KH=2, KW=2, stride=2, pad=0, M1=Co, Nc=Ci, a1=ptr(gf), b=ptr(x),
             slab=ptr(slab), splits=splits)
    if dims == 3:
        d.update(QD=Hc, AD=2 * Hc, KD=2)
    C().f32_wgrad(d, stream())
    torch.cuda.synchronize()
    X.assert_bits_equal(slab.double().sum(0), case.ref["gk"].reshape(T, Co, Ci), "fp32 tconv weight gradient")
    report("f32 tconv dims=%d" % dims, "f32_conv/f32_wgrad", case, case.ref["y"], t0)


# ---------------------------------------------------------------------------- coverage
def test_cases_cover_every_window_image_and_first_layer_kernel(cuda_dev):
    """The dicts above dispatch to conv_fwd_pick ids 6, 9, 10, 11, 12, 13 and 14 and to the
    32-, 64- and 128-wide-Cout implicit-GEMM tiles (4, 2, 1)."""
    P = collections.defaultdict(lambda: 1)
    hit = set()
    for dtype, key in FWD:
        hit.add(C().conv_fwd_pick(fwd_dict(key, P)))
    for N, H, Ci, Co, tile, _ in TCONV:
        hit.update(C().conv_fwd_pick(d) for d in tconv_dicts(N, H, Ci, Co, tile, P))
    for (N, D, H, C1, C2, Co, dtype), tile, bits, _ in DGRAD:
        hit.add(C().conv_fwd_pick(dgrad_dict(N, D, H, C1, C2, Co, tile, P, bits, 1.25)))
    for N, nsplit, mask in X.CONV_DW:
        hit.add(C().conv_fwd_pick(conv_dw_dict(N, nsplit, mask, P)))
    assert {6, 9, 10, 11, 12, 13, 14} <= hit, hit
    forced = {key[7] for _, key in FWD if key[7] in (1, 2, 4)}
    assert forced == {1, 2, 4}
    assert {1, 2, 4} <= hit, hit
